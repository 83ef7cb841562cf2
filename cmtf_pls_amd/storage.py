"""16-bit storage of X (bfloat16 / float16): how it is read and what the reports say about it, decided here alone.
A routine reads the 16-bit tensor itself through the _bf16 / _f16 form of an entry, or an exact float32 upcast of the rounded data (a
private copy), and its report says which, and why.  Four parts; nothing of the package is imported, so every module may import this one:
  types     HALF_DTYPES, SUFFIX, read_dtype, dtype_name, entry_name; the uploads that round once (to_device_copy, to_device_read)
  table     HALF_ENTRIES: the entries with 16-bit forms, grouped by who reads through them; HALF_ALWAYS_UPCAST: the routines that copy
  route     half_route: in place, or (upcast, why) -- the only probe of a backend's has_half
  recorder  StorageNotes on `pls._storage`, installed by the decorator reports_storage, which writes the routine's report"""
from __future__ import annotations

import functools
from typing import Optional

import numpy as np
import torch

# 16-bit storage of X (chosen explicitly with dtype=, never by dtype=None): X is only ever READ in that type -- the cross-covariance
# fit and the one-pass projection convert on load; every step that would write X or has no 16-bit form runs on an exact float32 upcast.
HALF_DTYPES = (torch.bfloat16, torch.float16)
SUFFIX = {torch.float32: "f32", torch.float64: "f64", torch.bfloat16: "bf16", torch.float16: "f16"}      # of an entry's name


def read_dtype(dtype):             # the type the routines without a 16-bit form read a model's X in: an exact upcast of 16-bit storage
    return torch.float32 if dtype in HALF_DTYPES else dtype


def dtype_name(dtype: torch.dtype) -> str:                 # "bfloat16", "float32", ...: a storage type as the reports name it
    return str(dtype).replace("torch.", "")


def entry_name(base: str, dtype: torch.dtype) -> str:      # the form of entry `base` that reads X of type `dtype`
    return f"cmtfpls_{base}_{SUFFIX[dtype]}"


def _as_torch_dtype(dtype, like) -> torch.dtype:
    """Storage type of X on the GPU: explicit, or float32 only when the input already is float32."""
    if dtype is None:
        return torch.float32 if like.dtype in (np.float32, torch.float32) else torch.float64
    if isinstance(dtype, torch.dtype):
        return dtype
    name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
    return {n: d for d, suffix in SUFFIX.items() for n in (dtype_name(d), suffix)}[name]           # "float32" or "f32", ...


# the entries that have _bf16 / _f16 forms, by who reads X through them: the fit's statistics read, one-read and two-read passes; the
# projection's score pass; the resampling drivers' three builders of S, score pass and contraction; the read-only diagnostics passes
HALF_ENTRIES = {
    "fit": ("xcov", "xcov_stats", "score_contract", "mttkrp"),
    "projection": ("mttkrp",),
    "folds": ("kfold_xcov", "kfold_wide_xcov", "kfold_weighted_xcov", "mttkrp", "xcov"),
    "diagnostics": ("recon_r2", "resid_rows", "contrib_rows", "selectivity_cols"),
}
# the routines that copy 16-bit storage whatever the options say, and why (the report's storage_fallback)
HALF_ALWAYS_UPCAST = {
    "impute": "impute returns a float32 tensor of X's size either way, so reading the 16-bit tensor in place would save nothing",
    "q2x_heldout": "get_q2x_heldout refits masked copies of X, and the refit writes them",
}


def half_route(owner, option: Optional[str], entries):
    """How `owner` (a model, or its engine) reads 16-bit X through `entries` (names of the table; for impute / get_q2x_heldout the
    routine's): (True, None) = the 16-bit tensor itself; (False, why) = a float32 upcast for that reason.  `option`: the EngineOptions
    switch that governs (None: the fit and the projection, which always try); while it is off the answer is (False, None): the routine's
    general reason then stands, and every bit and report text is that of a model without the option."""
    eng = owner._get_engine() if hasattr(owner, "_get_engine") else owner
    if option is not None and not getattr(eng.opt, option, False):
        return False, None
    pre = f"EngineOptions.{option}: " if option else ""
    for e in entries:
        if e in HALF_ALWAYS_UPCAST:
            return False, pre + HALF_ALWAYS_UPCAST[e]
    be = eng.be
    missing = [e for e in entries if not (hasattr(be, "has_half") and be.has_half(e))]
    if missing:
        return False, (f"{pre}the {getattr(be, 'name', type(be).__name__)} backend has no 16-bit form of "
                       + ", ".join(f"cmtfpls_{e}_*" for e in missing))
    return True, None


# why a routine without 16-bit reads copies 16-bit storage, unless its reads give reasons of their own
ROUTINE_WHY = "the kernels of this routine have no 16-bit form and read an exact float32 upcast of the rounded data"
FOLDS_WHY = "the fold and resampling kernels have no 16-bit form and read an exact float32 upcast of the rounded data"


def fallback_text(names, why: str) -> str:                 # the report's sentence for a float32 copy of data of the types `names`
    return f"float32 private copy of the {' / '.join(sorted(set(names)))} data: {why}"


class StorageNotes:
    """What one routine did with the 16-bit blocks it read, for its report.  Other types are not noted."""

    def __init__(self):
        self.upcasts, self.whys, self.reads = [], [], []      # type names; the reads' own reasons, first seen first; (type name, entries)

    def upcast(self, dtype: torch.dtype, why: Optional[str] = None) -> None:
        """A private upcast of a block of type `dtype` was read, for this read's own reason `why` (else the routine's general one)."""
        if dtype in HALF_DTYPES:
            self.upcasts.append(dtype_name(dtype))
            if why is not None and why not in self.whys:
                self.whys.append(why)

    def in_place(self, dtype: torch.dtype, entries) -> None:
        """A block of type `dtype` was read as it is, through its form of `entries` (names of the table)."""
        if dtype in HALF_DTYPES:
            self.reads.append((dtype_name(dtype), tuple(entry_name(e, dtype) for e in entries)))

    def declined(self, Xd, forms) -> None:
        """The per-block `forms` of a pass over Xd: a 16-bit block whose kernel declined was upcast (ProjectionMixin._fallback_block)."""
        for X, f in zip(Xd, forms):
            if f.get("why"):
                self.upcast(X.dtype, f["why"])

    def merge(self, inner: "StorageNotes") -> None:             # the notes of a routine that ran inside this one are this one's too
        self.upcasts.extend(inner.upcasts)
        self.whys.extend(w for w in inner.whys if w not in self.whys)
        self.reads.extend(inner.reads)

    def write(self, report, general_why: str) -> None:
        """An upcast wins: "storage_fallback", with the reads' own reasons where they gave any; "half_storage" when every read was in
        place and the report shows reads of X."""
        if self.upcasts and isinstance(report, dict):
            report["storage_fallback"] = fallback_text(self.upcasts, "; ".join(self.whys) or general_why)
        elif self.reads and isinstance(report, dict) and report.get("x_reads") is not None:
            report["half_storage"] = {"in_place": True, "dtype": " / ".join(sorted({d for d, _ in self.reads})),
                                      "entries": sorted({e for _, es in self.reads for e in es})}


def notes_of(pls) -> StorageNotes:  # of the routine running on `pls`; outside a routine that reports (or without a model) nobody reads them
    return getattr(pls, "_storage", None) or StorageNotes()


def reports_storage(report_attr: str, why: str = ROUTINE_WHY):
    """Decorator of a routine `fn(pls, ...)` that leaves its report in `pls.<report_attr>`: its reads of 16-bit X are noted in
    `pls._storage` and written to the report when it returns (`why`: the general reason); an inner routine's notes are the outer's too."""
    def deco(fn):
        @functools.wraps(fn)
        def run(pls, *args, **kw):
            outer, notes = getattr(pls, "_storage", None), StorageNotes()
            pls._storage = notes
            try:
                out = fn(pls, *args, **kw)
            finally:
                pls._storage = outer
            notes.write(getattr(pls, report_attr, None), why)
            if outer is not None:
                outer.merge(notes)
            return out
        return run
    return deco


def _round_once(x64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 -> bfloat16 / float16 with ONE rounding to nearest even, on any device.  A plain cast goes through float32 and
    rounds twice (about 1 value in 20000 then differs from the correctly rounded one).  Here the float32 step rounds to ODD
    (truncate towards zero, set the last bit when anything was lost), which keeps what the final rounding needs to know; the
    float32 -> 16-bit cast is then a single rounding of the right value (float32 has more than two bits to spare)."""
    f = x64.to(torch.float32)
    back = f.to(torch.float64)
    lost = (back != x64) & torch.isfinite(x64)
    bits = f.view(torch.int32)
    bits = torch.where(lost & (back.abs() > x64.abs()), bits - 1, bits)      # sign-magnitude: one less is one step towards zero
    bits = torch.where(lost, bits | 1, bits)
    return bits.view(torch.float32).to(dtype)


def _half_from_f64(src: torch.Tensor, dtype: torch.dtype, device) -> torch.Tensor:
    """A float64 tensor (host or device) as a fresh 16-bit device tensor, rounded once, in row blocks of <= 256 MB."""
    out = torch.empty(src.shape, dtype=dtype, device=device)
    if src.ndim == 0:
        return out.copy_(_round_once(src.to(device), dtype))
    rows = max(1, (256 << 20) // max(src[0].numel() * 8, 1))
    for r in range(0, src.shape[0], rows):
        out[r:r + rows].copy_(_round_once(src[r:r + rows].to(device), dtype))
    return out


def to_device_copy(X, dtype: torch.dtype, device, copy: bool = True) -> torch.Tensor:
    """A fresh contiguous device tensor of X (inputs are never modified, tpls.py:74,128,151).
    copy=False (opt-in ``copy_X=False``): a device tensor that already has the right type is used in
    place and is centred / deflated by the fit.

    A large HOST array of another type than the storage type (the common case: float64 NumPy input, float32
    storage) is shipped in row blocks in ITS OWN type and cast on the device: casting 8.6 GB on the host first costs
    ~0.75 s at 65536 x 128 x 128, the extra PCIe bytes ~0.08 s (profiles/r02aa_pcie_inclusive.txt)."""
    if isinstance(X, torch.Tensor):
        if not copy and X.is_contiguous() and X.dtype == dtype and X.device == torch.device(device):
            return X
        if dtype in HALF_DTYPES and X.dtype == torch.float64:
            return _half_from_f64(X.contiguous(), dtype, device)     # one rounding, whatever the container (as NumPy's astype)
        out = X.to(device=device, dtype=dtype, copy=True)
        return out.contiguous()
    Xn = np.ascontiguousarray(X)
    src = torch.from_numpy(Xn)
    if dtype in HALF_DTYPES and src.dtype == torch.float64:
        return _half_from_f64(src, dtype, device)                    # the stored data is X.astype(np.float16), not a double rounding
    if src.dtype == dtype or Xn.ndim == 0 or Xn.nbytes < (64 << 20):
        return src.to(device=device, dtype=dtype, copy=True).contiguous()
    out = torch.empty(Xn.shape, dtype=dtype, device=device)
    rows = max(1, (256 << 20) // max(Xn[0].nbytes, 1))           # ~256 MB of the source type per block
    for r in range(0, Xn.shape[0], rows):
        out[r:r + rows].copy_(src[r:r + rows].to(device))        # H2D in the source type, cast by the device copy
    return out


def to_device_read(X, dtype: torch.dtype, device, pls=None, why: Optional[str] = None, entry: Optional[str] = None) -> torch.Tensor:
    """X on the device as the routines beside fit / transform read it: `to_device_copy(X, dtype, device, copy=False)` -- and for a
    model with 16-bit storage the data ROUNDED to that type, then upcast to float32: exactly the values the model was fitted on, in a
    type those kernels take.  `pls`: the model on whose behalf X is read; the upcast is noted on it, with this read's own reason `why`
    where it has one.  `entry`: the kernel (or, for impute / get_q2x_heldout, the routine) that reads X, routed by half_route under
    EngineOptions.half_diagnostics: in place, the 16-bit tensor itself comes back (the caller's own, or the once-rounded upload)."""
    Xd = to_device_copy(X, dtype, device, copy=False)
    if dtype not in HALF_DTYPES:
        return Xd
    if entry is not None and pls is not None and why is None:
        in_place, why = half_route(pls, "half_diagnostics", (entry,))
        if in_place:
            notes_of(pls).in_place(dtype, (entry,))
            return Xd
    notes_of(pls).upcast(dtype, why)
    return Xd.to(torch.float32)
