"""HipBackend: the per-GPU kernel set of the NIPALS engine, one method per reference call site.

Every method launches hand-written gfx950 kernels from libcmtfpls.so (include/cmtfpls.h) on the
current torch stream; torch is used only to own device memory and the stream.  There is no CPU
path: constructing the backend without a GPU or without the library raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from .storage import HALF_DTYPES, HALF_ENTRIES, SUFFIX, entry_name

# the entries that have _bf16 / _f16 forms, each once: 16-bit X is only ever read, converted to f64 on load
_HALF_ENTRIES = tuple(dict.fromkeys(e for group in HALF_ENTRIES.values() for e in group))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _int_pairs(pairs):
    """A host int array of the flattened pairs (the `dims` of cmtfpls_kfold_inner_coupled_tensor_f64)."""
    flat = [int(v) for p in pairs for v in p]
    return (ctypes.c_int * len(flat))(*flat)


def _scratch(nbytes: int, device) -> torch.Tensor:
    """A byte buffer for a workspace: at least nbytes, never empty."""
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def chunk_size(n: int, per: int, budget: int, cap: Optional[int] = None) -> int:
    """Items per launch of a chunked workgroup-per-item call: as many of the n items as `budget` bytes hold at `per` bytes each,
    at least one, at most `cap`."""
    chunk = max(1, min(int(n), int(budget) // max(int(per), 1)))
    return chunk if cap is None else min(chunk, int(cap))


class HipBackend:
    name = "hip"

    def __init__(self, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CmtfplsError("cmtf_pls_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.n_partials = int(self.lib.cmtfpls_sweep_partials())
        self._ws = {}
        self._status_slots = {}        # (slot, words) -> pinned host buffer + event of status_snapshot
        self.rank1_squarings = 30      # budget ceiling: resolves sigma_2/sigma_1 up to 1 - 1e-8
        # min(A, B) up to which cmtfpls_rank1_* runs all squarings in one launch (csrc/rank1.hip); 0 once the process switched it off
        self.rank1_chain_side = 256 if self.lib.cmtfpls_rank1_chain_enabled() else 0

    # -- helpers ---------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _workspace(self, key: str, nbytes: int) -> torch.Tensor:
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = self._ws[key] = _scratch(nbytes, self.device)
        return buf

    @staticmethod
    def _form(rc: int, name: str, value=True):
        """The answer of an entry that may decline the shape: None on status 4, else `value` once the status is checked."""
        if rc == 4:
            return None
        _lib.check(rc, name)
        return value

    def _chunked_launch(self, name: str, call, n: int, per_fn, budget: int, cap: Optional[int] = None, extra: int = 0,
                        ws_key: Optional[str] = None) -> Optional[int]:
        """Run call(first, count, ws_ptr, ws_bytes) -> status over the n items (folds, models) of a workgroup-per-item entry point
        in chunks whose workspace fits `budget` bytes; the number of launches, or None when the entry point declines the shape
        (status 4).  The probe without a workspace comes first: the shape check precedes the workspace check (status 2).
        per_fn() gives the workspace bytes per item; `extra`: further bytes per item counted against the budget; `cap`: most items
        per launch; ws_key: the cached workspace to use (allocated for this call and released with it otherwise)."""
        if call(0, 1, None, 0) == 4:
            return None
        per = int(per_fn())
        chunk = chunk_size(n, per + extra, budget, cap)
        ws = self._workspace(ws_key, per * chunk) if ws_key else _scratch(per * chunk, self.device)
        launches = 0
        for i0 in range(0, n, chunk):
            if self._form(call(i0, min(chunk, n - i0), _ptr(ws), ws.numel()), name) is None:
                return None
            launches += 1
        return launches

    def _ws_budget(self, max_ws_bytes: Optional[int], third_of_free: bool = False) -> int:
        """The workspace budget of a chunked call: the caller's, else 4 GiB (third_of_free: or a third of the free HBM if more)."""
        if max_ws_bytes is not None:
            return int(max_ws_bytes)
        return max(4 << 30, torch.cuda.mem_get_info(self.device)[0] // 3) if third_of_free else 4 << 30

    def clear_error(self) -> bool:
        """After a failed HIP-graph capture: reset the runtime's pending error so that the next launch is not blamed for it."""
        return bool(self.lib.cmtfpls_clear_error())

    def empty(self, *shape, dtype=torch.float64) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=torch.float64) -> torch.Tensor:
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def has_half(self, base: str) -> bool:
        """Whether entry `base` has a form for 16-bit storage (bfloat16 / float16): the read-only passes over X only."""
        return base in _HALF_ENTRIES and all(hasattr(self.lib, entry_name(base, d)) for d in HALF_DTYPES)

    def _read_fn(self, base: str, X: torch.Tensor, mixed: bool = False):
        """The entry `base` for this X (`mixed`: its f32-MFMA form for f32-stored X); None when X is 16-bit and the entry has no such
        form, or `mixed` is asked: the caller declines, and 16-bit X is read through a float32 copy."""
        if X.dtype not in SUFFIX:
            raise TypeError(f"X must be float32 or float64 on device, got {X.dtype}")
        if X.dtype in HALF_DTYPES and (mixed or not self.has_half(base)):
            return None
        if mixed and X.dtype == torch.float32:
            return getattr(self.lib, f"cmtfpls_{base}_f32_mixed")
        assert X.is_contiguous() and X.device == self.device
        return getattr(self.lib, entry_name(base, X.dtype))

    def _fn(self, base: str, X: torch.Tensor):
        fn = self._read_fn(base, X)
        if fn is None:
            raise TypeError(f"{base} has no form for {X.dtype} storage (16-bit X is only read by {', '.join(_HALF_ENTRIES)}); "
                            "use a float32 copy")
        return fn

    def _close_partials(self, part: torch.Tensor) -> torch.Tensor:
        out = self.empty(1)
        _lib.check(self.lib.cmtfpls_sum_f64(_ptr(part), part.numel(), _ptr(out), self._stream()), "sum")
        return out

    # -- which kernel instance and grid policy a sweep takes (host arithmetic, no GPU call) ------
    @staticmethod
    def sweep_form(op: str, dtype, I: int, A: int, B: int, masked: bool = False, M: int = 0, aligned16: bool = True) -> str:
        """Name of the form the X sweep `op` takes for an (I, A * B) block of `dtype` (cmtfpls_sweep_form); a shape the entry
        declines gives "unsupported: <reason>".  Needs the library but no device."""
        buf = ctypes.create_string_buffer(256)
        elem = 4 if dtype in (torch.float32, "f32", "float32") else 8
        _lib.check(_lib.load().cmtfpls_sweep_form(op.encode(), elem, int(I), int(A), int(B), int(bool(masked)), int(M), int(bool(aligned16)),
                                                  buf, len(buf)), "sweep_form")
        return buf.value.decode()

    @staticmethod
    def sweep_form_list(op: str, dtype) -> list:
        """Every name sweep_form can give for `op` and `dtype` (cmtfpls_sweep_form_list)."""
        buf = ctypes.create_string_buffer(1 << 14)
        elem = 4 if dtype in (torch.float32, "f32", "float32") else 8
        _lib.check(_lib.load().cmtfpls_sweep_form_list(op.encode(), elem, buf, len(buf)), "sweep_form_list")
        return buf.value.decode().splitlines()

    # -- measured HBM ceilings (bench.py: roofline denominators measured in the same run) ---------
    def ceiling(self, op: str, buf: torch.Tensor, row_bytes: int = 0, blocks: int = 2048,
                dst: Optional[torch.Tensor] = None, map: int = 0) -> bool:
        """op: "read" | "rmw" (negates in place; call an even number of times) | "copy" (needs dst); map: 0 flat,
        1 chunked, 2 row per 1024-thread workgroup with a barrier, 3 column owner.  False when the map does not take the shape."""
        nbytes = buf.numel() * buf.element_size()
        if op == "read":
            sink = self._workspace("ceiling_sink", 4 * self.lib.cmtfpls_ceiling_max_blocks())
            rc = self.lib.cmtfpls_ceiling_read(_ptr(buf), nbytes, int(row_bytes), int(map), _ptr(sink), int(blocks), self._stream())
        elif op == "rmw":
            rc = self.lib.cmtfpls_ceiling_rmw(_ptr(buf), nbytes, int(row_bytes), int(map), int(blocks), self._stream())
        elif op == "copy":
            assert dst is not None and dst.numel() * dst.element_size() >= nbytes
            rc = self.lib.cmtfpls_ceiling_copy(_ptr(buf), _ptr(dst), nbytes, int(row_bytes), int(map), int(blocks), self._stream())
        else:
            raise ValueError(op)
        return self._form(rc, "ceiling_" + op, False) is not None

    # -- preprocess: tpls.py:61-71 -----------------------------------------------------------
    def colstats(self, X2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        I, P = X2.shape
        ws = self._workspace("contract", self.lib.cmtfpls_colstats_workspace_bytes(I, P))
        colsum, colcnt = self.empty(P), self.empty(P)
        _lib.check(self._fn("colstats", X2)(_ptr(X2), I, P, _ptr(colsum), _ptr(colcnt), _ptr(ws), ws.numel(), self._stream()), "colstats")
        return colsum, colcnt

    def center(self, X2: torch.Tensor, mean: torch.Tensor, want_rowcnt: bool) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        I, P = X2.shape
        rowcnt = self.empty(I) if want_rowcnt else None
        part = self.empty(self.n_partials)
        _lib.check(self._fn("center", X2)(_ptr(X2), I, P, _ptr(mean), _ptr(rowcnt), _ptr(part), self._stream()), "center")
        return rowcnt, self._close_partials(part)

    # -- K1: tpls.py:83 / missingvals.py:7-20 ------------------------------------------------
    def mode0_contract(self, X2: torch.Tensor, u: torch.Tensor, masked: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        I, P = X2.shape
        ws = self._workspace("contract", self.lib.cmtfpls_mode0_contract_workspace_bytes(I, P))
        Z = out if out is not None else self.empty(P)
        _lib.check(self._fn("mode0_contract", X2)(_ptr(X2), I, P, _ptr(u), _ptr(Z), int(masked), _ptr(ws), ws.numel(), self._stream()), "mode0_contract")
        return Z

    def mode0_contract_yq(self, X2: torch.Tensor, Y: torch.Tensor, q: torch.Tensor, masked: bool,
                          out: torch.Tensor) -> Optional[torch.Tensor]:
        """Z = X x_0 (Y q) with u = Y q (tpls.py:102) formed inside the kernel; None when the shape is outside
        the fused form (caller: rowdot + mode0_contract)."""
        I, P = X2.shape
        ws = self._workspace("contract", self.lib.cmtfpls_mode0_contract_workspace_bytes(I, P))
        rc = self._fn("mode0_contract_yq", X2)(_ptr(X2), I, P, _ptr(Y), Y.stride(0), Y.shape[1], _ptr(q), _ptr(out), int(masked),
                                               _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "mode0_contract_yq", out)

    def colscale(self, Z: torch.Tensor, colcnt: torch.Tensor, n_samples: float) -> None:
        _lib.check(self.lib.cmtfpls_colscale_f64(_ptr(Z), Z.numel(), _ptr(colcnt), float(n_samples), self._stream()), "colscale")

    # -- K2: tpls.py:84-90 -------------------------------------------------------------------
    def rank1(self, Z: torch.Tensor, A: int, B: int, wA: torch.Tensor, wB: torch.Tensor,
              info: Optional[torch.Tensor] = None, n_squarings: Optional[int] = None, launches: bool = False) -> None:
        """info (2 doubles, optional): [converged within the budget, squarings computed].  launches: the launch-per-squaring
        form (cmtfpls_rank1_launches_f64) instead of the one-launch chain the entry takes for min(A, B) <= 256 -- same bits."""
        ws = self._workspace("rank1", self.lib.cmtfpls_rank1_workspace_bytes(A, B))
        fn = self.lib.cmtfpls_rank1_launches_f64 if launches else self.lib.cmtfpls_rank1_f64
        _lib.check(fn(_ptr(Z), A, B, _ptr(wA), _ptr(wB), None, _ptr(info), int(n_squarings or self.rank1_squarings),
                      _ptr(ws), ws.numel(), self._stream()), "rank1")

    def rank1_chain_gave_up(self) -> None:
        """An extraction reported info = [0, -1]: a workgroup of the one-launch chain of squarings never became resident (the GPU
        is shared with another process).  From here on every entry of this process takes the launch-per-squaring form."""
        self.lib.cmtfpls_rank1_chain_enable(0)
        self.rank1_chain_side = 0

    def rank1_tensor(self, Z: torch.Tensor, dims, tol: float, factors: torch.Tensor,
                     info: Optional[torch.Tensor] = None, n_squarings: Optional[int] = None) -> None:
        """Rank-1 CP factors of a cross-covariance tensor of order 3 to 7 (X of order 4 to 8), every mode <= 1024; factors: (n, ld)
        f64, row m = mode m.  info (2 doubles, optional): [1, ALS sweeps run], or [0, -1] with NaN factors when the one-launch
        chain of squarings of an init gave up (as rank1 reports it: rank1_chain_gave_up, then call again)."""
        arr = (ctypes.c_int * len(dims))(*[int(d) for d in dims])
        ws = self._workspace("rank1t", self.lib.cmtfpls_rank1_tensor_workspace_bytes(arr, len(dims)))
        _lib.check(self.lib.cmtfpls_rank1_tensor_f64(_ptr(Z), arr, len(dims), float(tol), _ptr(factors), factors.stride(0), _ptr(info),
                                                     int(n_squarings or self.rank1_squarings), _ptr(ws), ws.numel(), self._stream()),
                   "rank1_tensor")

    def kron(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        _lib.check(self.lib.cmtfpls_kron_f64(_ptr(a), a.numel(), _ptr(b), b.numel(), _ptr(out), self._stream()), "kron")
        return out

    def normalize(self, v: torch.Tensor) -> None:
        _lib.check(self.lib.cmtfpls_normalize_f64(_ptr(v), v.numel(), None, self._stream()), "normalize")

    # -- sparse loadings: soft-thresholded sweeps on the dense pair (csrc/rank1_sparse.hip) ------------------------
    def rank1_sparse_form(self, A: int, B: int) -> int:
        """1: Z staged in LDS once; 2: Z streamed on every half-sweep; 0: outside 2 <= A, B <= 4096, A * B <= 65536."""
        return int(self.lib.cmtfpls_rank1_sparse_form(int(A), int(B)))

    def rank1_sparsify(self, Z: torch.Tensor, A: int, B: int, wA: torch.Tensor, wB: torch.Tensor, lamA: float, lamB: float,
                       info: Optional[torch.Tensor] = None, tol_s: float = 1e-10, max_sweeps: int = 200) -> None:
        """(wA, wB): the dense pair of Z in, the soft-thresholded pair out, every sweep in ONE launch of one workgroup.
        info (2 doubles, optional): [converged, sweeps run]."""
        _lib.check(self.lib.cmtfpls_rank1_sparse_f64(_ptr(Z), int(A), int(B), _ptr(wA), _ptr(wB), float(lamA), float(lamB), float(tol_s),
                                                     int(max_sweeps), _ptr(info), None, 0, self._stream()), "rank1_sparse")

    def soft_normalize(self, v: torch.Tensor, lam: float) -> None:
        """v <- soft(v, lam) / |soft(v, lam)|_2 in place: the loading of a matrix block with sparsity."""
        _lib.check(self.lib.cmtfpls_soft_normalize_f64(_ptr(v), v.numel(), float(lam), None, self._stream()), "soft_normalize")

    # -- cross-covariance form (exact re-association of the loop, see include/cmtfpls.h) --------
    def xcov(self, X2: torch.Tensor, Y: torch.Tensor, masked: bool, out: Optional[torch.Tensor] = None,
             mixed: bool = False) -> Optional[torch.Tensor]:
        """S (M, P) = Y^T X_(0) on the matrix cores (f64 MFMA; ``mixed`` = the opt-in f32-MFMA form for
        f32-stored X).  More than 64 responses: tiles of 64, one pass over X each (inside the C entry)."""
        I, P = X2.shape
        M = Y.shape[1]
        fn = self._read_fn("xcov", X2, mixed)
        if fn is None:
            return None
        ws = self._workspace("contract", self.lib.cmtfpls_xcov_workspace_bytes(I, P, M))
        S = out if out is not None else self.empty(M, P)
        _lib.check(fn(_ptr(X2), I, P, _ptr(Y), Y.stride(0), M, _ptr(S), int(masked), _ptr(ws), ws.numel(), self._stream()), "xcov")
        return S

    def xcov_deflate(self, X2: torch.Tensor, A: int, B: int, Y: torch.Tensor, t: torch.Tensor, wA: torch.Tensor, wB: torch.Tensor,
                     out: torch.Tensor) -> Optional[torch.Tensor]:
        """X -= t (x) w in place AND S = Y^T X0 of the deflated block (NaN -> 0) AND |X0|^2, one read + write of X
        (cmtfpls_xcov_deflate_*).  Returns the norm (one-element device tensor); None when the shape is outside the kernel
        (nothing written: deflate, then xcov)."""
        I, P = X2.shape
        M = Y.shape[1]
        if M > 64 or P % 4 != 0 or P != A * B:
            return None
        ws = self._workspace("contract", self.lib.cmtfpls_xcov_ssq_workspace_bytes(I, P, M))
        ssq = self.empty(1)
        rc = self._fn("xcov_deflate", X2)(_ptr(X2), I, A, B, _ptr(Y), Y.stride(0), M, _ptr(t), _ptr(wA), _ptr(wB), _ptr(out), _ptr(ssq),
                                          _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "xcov_deflate", ssq)

    def rank1_score(self, Z: torch.Tensor, A: int, B: int, wA: torch.Tensor, wB: torch.Tensor, S: torch.Tensor, tq: torch.Tensor,
                    info: Optional[torch.Tensor] = None, n_squarings: Optional[int] = None) -> torch.Tensor:
        """rank1(Z) -> (wA, wB), then tq = S (wA (x) wB) for the M rows of S, the extraction's last kernel and the score in one
        launch where the shape allows (cmtfpls_rank1_score_f64)."""
        M = S.shape[0]
        assert S.is_contiguous() and S.shape[1] == A * B and tq.numel() >= M
        ws = self._workspace("rank1", self.lib.cmtfpls_rank1_workspace_bytes(A, B))
        _lib.check(self.lib.cmtfpls_rank1_score_f64(_ptr(Z), A, B, _ptr(wA), _ptr(wB), _ptr(info),
                                                    int(n_squarings if n_squarings is not None else self.rank1_squarings),
                                                    _ptr(S), M, _ptr(tq), _ptr(ws), ws.numel(), self._stream()), "rank1_score")
        return tq

    def xcov_ssq(self, X2: torch.Tensor, Y: torch.Tensor, mean: torch.Tensor, out: torch.Tensor):
        """S = Y^T X_(0) AND sum (X - mean)^2 from one read of an uncentred, NaN-free X (cmtfpls_xcov_ssq_*); returns
        (S, ssq as a one-element device tensor).  More than 64 responses: tiles of 64, the norm from the first pass."""
        I, P = X2.shape
        M = Y.shape[1]
        ws = self._workspace("contract", self.lib.cmtfpls_xcov_ssq_workspace_bytes(I, P, M))
        ssq = self.empty(1)
        assert mean.is_contiguous() and mean.numel() == P and mean.dtype == torch.float64
        _lib.check(self._fn("xcov_ssq", X2)(_ptr(X2), I, P, _ptr(Y), Y.stride(0), M, _ptr(out), _ptr(mean), _ptr(ssq), _ptr(ws), ws.numel(),
                                            self._stream()), "xcov_ssq")
        return out, ssq

    def xcov_stats(self, X2: torch.Tensor, Y: torch.Tensor, out: torch.Tensor):
        """S = Y^T X_(0) AND the column sums / sums of squares of an uncentred X from ONE read (cmtfpls_xcov_stats_*): returns
        (S, stats) with stats[:P] the sums and stats[P:] the sums of squares, or None for more than 64 responses."""
        I, P = X2.shape
        M = Y.shape[1]
        fn = self._read_fn("xcov_stats", X2) if M <= 64 and X2.is_contiguous() else None
        if fn is None:
            return None
        ws = self._workspace("contract", self.lib.cmtfpls_xcov_stats_workspace_bytes(I, P, M))
        stats = self.empty(2 * P)
        rc = fn(_ptr(X2), I, P, _ptr(Y), Y.stride(0), M, _ptr(out), _ptr(stats), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "xcov_stats", (out, stats))

    def status_snapshot(self, status: torch.Tensor, slot: int, slots: Optional[dict] = None):
        """Enqueue a copy of a few status words to pinned host memory behind the work issued so far (cmtfpls_status_to_host);
        returns a token for status_wait.  (slot: the caller keeps at most one snapshot per slot in flight.)  `slots`: the
        CALLER's cache of pinned buffers and events -- a fit in flight owns its own (FitRun._pipe), so two fits on one
        backend (other threads, other streams) never share a buffer; None: the backend's own, for single-threaded tools."""
        slots = self._status_slots if slots is None else slots
        ent = slots.get((slot, status.numel()))
        if ent is None:
            host, ev = torch.empty(status.numel(), dtype=torch.float64, pin_memory=True), torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))               # (creates the underlying hipEvent_t)
            ent = slots[(slot, status.numel())] = (host, ev, host.numpy(), host.data_ptr(), ev.cuda_event, status.numel() * 8)
        rc = self.lib.cmtfpls_status_to_host(status.data_ptr(), ent[3], ent[5], ent[4], self._stream())
        if rc:
            _lib.check(rc, "status_to_host")
        return ent

    def status_wait(self, token) -> "np.ndarray":
        token[1].synchronize()
        return token[2]

    def xcov_iterate_plan(self, S: torch.Tensor, A: int, B: int, q_cur: torch.Tensor, Z: torch.Tensor, wA: torch.Tensor,
                          wB: torch.Tensor, status: torch.Tensor, q_new: torch.Tensor, G: torch.Tensor):
        """xcov_iterate on fixed buffers with its arguments marshalled ONCE: returns enqueue(n_squarings, first).  (The inner
        loop on S is ~15 launches of a few microseconds; per-call argument handling in Python was a tenth of an iteration.)"""
        M, P = S.shape
        wc = self._workspace("contract", self.lib.cmtfpls_mode0_contract_workspace_bytes(M, P))
        wr = self._workspace("rank1", self.lib.cmtfpls_rank1_workspace_bytes(A, B))
        keep = (S, q_cur, Z, wA, wB, status, q_new, G, wc, wr)                 # the plan owns references: pointers stay valid
        fn = self.lib.cmtfpls_xcov_iterate_f64
        head = (_ptr(S), M, A, B, _ptr(q_cur), _ptr(Z), _ptr(wA), _ptr(wB), status[1:3].data_ptr())
        tail = (_ptr(wc), wc.numel(), _ptr(wr), wr.numel())
        qn, Gp, du2 = _ptr(q_new), _ptr(G), status[0:1].data_ptr()
        stream = self._stream

        def enqueue(n_squarings: int, first: bool, _keep=keep) -> None:
            rc = fn(*head, n_squarings, qn, Gp, du2, 1 if first else 0, *tail, stream())
            if rc:
                _lib.check(rc, "xcov_iterate")
        return enqueue

    def xcov_iterate(self, S: torch.Tensor, A: int, B: int, q_cur: torch.Tensor, Z: torch.Tensor, wA: torch.Tensor,
                     wB: torch.Tensor, info: torch.Tensor, n_squarings: int, q_new: torch.Tensor, G: torch.Tensor,
                     du2: torch.Tensor, first: bool) -> None:
        """One inner iteration on S (contraction, rank-1, score, norm, |du|^2) issued by one host call."""
        M, P = S.shape
        wc = self._workspace("contract", self.lib.cmtfpls_mode0_contract_workspace_bytes(M, P))
        wr = self._workspace("rank1", self.lib.cmtfpls_rank1_workspace_bytes(A, B))
        _lib.check(self.lib.cmtfpls_xcov_iterate_f64(_ptr(S), M, A, B, _ptr(q_cur), _ptr(Z), _ptr(wA), _ptr(wB), _ptr(info),
                                                     int(n_squarings), _ptr(q_new), _ptr(G), _ptr(du2), int(first),
                                                     _ptr(wc), wc.numel(), _ptr(wr), wr.numel(), self._stream()), "xcov_iterate")

    def xcov_blocks_plan(self, blocks, M: int, q_cur: torch.Tensor, tq: torch.Tensor, q_new: torch.Tensor, G: torch.Tensor,
                         status: torch.Tensor):
        """One inner iteration on S for SEVERAL coupled blocks / blocks with missing values (cmtfpls_xcov_iterate_blocks_f64) on fixed
        buffers, arguments marshalled once.  blocks: dicts with S, S2 (or None), colcnt (or None), n_samples, order (2 | 3), A, B,
        Z, wA, wB; status = [du2, (converged, squarings used) per block].  Returns enqueue(n_squarings per block, first), or
        None when a block is outside the entry (order > 3, M > 64)."""
        nb = len(blocks)
        if M > 64 or any(b["order"] not in (2, 3) for b in blocks) or tq.numel() != nb * M or not tq.is_contiguous():
            return None
        arr = (_lib.XcovBlock * nb)()
        need = 256
        for i, b in enumerate(blocks):
            for name in ("S", "S2", "colcnt", "Z", "wA", "wB"):
                t = b.get(name)
                assert t is None or (t.is_contiguous() and t.dtype == torch.float64 and t.device == self.device), name
                setattr(arr[i], name, _ptr(t))
            arr[i].n_samples, arr[i].order, arr[i].A, arr[i].B = float(b["n_samples"]), int(b["order"]), int(b["A"]), int(b["B"])
            arr[i].info = status[1 + 2 * i: 3 + 2 * i].data_ptr()
            if b["order"] == 3:
                need = max(need, self.lib.cmtfpls_rank1_workspace_bytes(b["A"], b["B"]))
        wr = self._workspace("rank1", need)
        keep = (blocks, q_cur, tq, q_new, G, status, wr, arr)                    # the plan owns references: pointers stay valid
        fn, stream = self.lib.cmtfpls_xcov_iterate_blocks_f64, self._stream
        args = (nb, M, _ptr(q_cur), _ptr(tq), _ptr(q_new), _ptr(G), status[0:1].data_ptr())
        tail = (_ptr(wr), wr.numel())

        def enqueue(n_squarings, first: bool, _keep=keep) -> None:
            for i in range(nb):
                arr[i].n_squarings = int(n_squarings[i])
            rc = fn(arr, *args, 1 if first else 0, *tail, stream())
            if rc:
                _lib.check(rc, "xcov_iterate_blocks")
        return enqueue

    def s_downdate(self, S: torch.Tensor, A: int, B: int, ya: torch.Tensor, wA: torch.Tensor, wB: torch.Tensor,
                   q: torch.Tensor, v: torch.Tensor) -> None:
        """S -= ya w^T + q v^T, w = kron(wA, wB): S = Y^T X_(0) carried across one deflation."""
        assert S.is_contiguous() and S.shape[1] == A * B
        _lib.check(self.lib.cmtfpls_s_downdate_f64(_ptr(S), S.shape[0], A, B, _ptr(ya), _ptr(wA), _ptr(wB), _ptr(q), _ptr(v),
                                                   self._stream()), "s_downdate")

    def kr_axpy(self, v: torch.Tensor, A: int, B: int, WA: torch.Tensor, WB: torch.Tensor, k: int, coef: torch.Tensor) -> torch.Tensor:
        """v (A*B) -= sum_{j<k} coef[j] * kron(WA[:, j], WB[:, j]); WA (A, R), WB (B, R) row-major."""
        assert WA.is_contiguous() and WB.is_contiguous() and WA.shape[1] == WB.shape[1] and coef.numel() >= k
        _lib.check(self.lib.cmtfpls_kr_axpy_f64(_ptr(v), A, B, _ptr(WA), _ptr(WB), WA.shape[1], int(k), _ptr(coef), self._stream()), "kr_axpy")
        return v

    def axpy_scalar(self, y: torch.Tensor, a: torch.Tensor, x: Optional[torch.Tensor] = None) -> torch.Tensor:
        """y -= a[0] * x (x = None: ones); a is a one-element device tensor."""
        assert y.is_contiguous() and y.dtype == torch.float64 and a.numel() >= 1 and (x is None or (x.is_contiguous() and x.numel() == y.numel()))
        _lib.check(self.lib.cmtfpls_axpy_scalar_f64(_ptr(y), y.numel(), _ptr(a), _ptr(x), self._stream()), "axpy_scalar")
        return y

    def total(self, v: torch.Tensor) -> torch.Tensor:
        """Sum of a contiguous f64 vector as a one-element device tensor (fixed-order, one workgroup)."""
        assert v.is_contiguous() and v.dtype == torch.float64
        return self._close_partials(v)

    def quadform(self, G: torch.Tensor, q: torch.Tensor, q_old: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        _lib.check(self.lib.cmtfpls_quadform_f64(_ptr(G), G.shape[0], _ptr(q), _ptr(q_old), _ptr(out), self._stream()), "quadform")
        return out

    def mttkrp(self, X2: torch.Tensor, A: int, B: int, WA: torch.Tensor, WB: torch.Tensor, out: torch.Tensor,
               mixed: bool = False) -> Optional[torch.Tensor]:
        """out (I, R) = X_(0) (WA (.) WB); None when R > 32 or the loadings do not fit LDS."""
        R = WA.shape[1]
        assert WA.is_contiguous() and WB.is_contiguous() and out.stride(1) == 1
        fn = self._read_fn("mttkrp", X2, mixed)
        if fn is None:
            return None
        rc = fn(_ptr(X2), X2.shape[0], A, B, _ptr(WA), _ptr(WB), R, _ptr(out), out.stride(0), self._stream())
        return self._form(rc, "mttkrp", out)

    # -- K3: tpls.py:92-99 / missingvals.py:23-38 --------------------------------------------
    def score(self, X2, A, B, wA, wB, rowcnt, out) -> torch.Tensor:
        _lib.check(self._fn("score", X2)(_ptr(X2), X2.shape[0], A, B, _ptr(wA), _ptr(wB), _ptr(rowcnt), _ptr(out), self._stream()), "score")
        return out

    def score_s(self, S, A, B, wA, wB, out) -> torch.Tensor:
        """out[m] = S[m, :] . kron(wA, wB) for the M rows of a cross-covariance S (or a one-row "tensor" such as the column
        means): cmtfpls_score_s_f64 -- few long rows take one workgroup each, which cmtfpls_score_* never does for samples."""
        assert S.dtype == torch.float64 and S.is_contiguous()
        _lib.check(self.lib.cmtfpls_score_s_f64(_ptr(S), S.shape[0], A, B, _ptr(wA), _ptr(wB), _ptr(out), self._stream()), "score_s")
        return out

    def score_contract(self, X2, A, B, wA, wB, shift, t, Z, sub_own=None, add_other=None, alpha: float = 1.0,
                       csum: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """t = X w - shift - sub_own and Z = X^T c, c = alpha (t + add_other), in one read of X (cmtfpls_score_contract_*); csum[0] =
        sum(c) when given; None when the row fits neither the registers of one workgroup nor those of 16 (the caller then makes the two passes)."""
        I, P = X2.shape
        fn = self._read_fn("score_contract", X2) if X2.is_contiguous() and P == A * B else None
        if fn is None:
            return None
        for v in (sub_own, add_other):
            assert v is None or (v.is_contiguous() and v.numel() == I and v.dtype == torch.float64)
        nbytes = self.lib.cmtfpls_score_contract_workspace_bytes(I, P)
        ws = self._workspace("score_contract", max(nbytes, 256))
        rc = fn(_ptr(X2), I, A, B, _ptr(wA), _ptr(wB), _ptr(shift), _ptr(sub_own), _ptr(add_other), float(alpha),
                                            _ptr(t), _ptr(Z), _ptr(csum), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "score_contract", Z)

    def score_gram(self, X2, A, B, wA, wB, rowcnt, out, Y: torch.Tensor, qpart: torch.Tensor) -> Optional[torch.Tensor]:
        """score + the per-workgroup partial sums of Y^T t into qpart (n_partials x M); None when M > 64."""
        assert qpart.numel() >= self.n_partials * Y.shape[1] and qpart.is_contiguous()
        rc = self._fn("score_gram", X2)(_ptr(X2), X2.shape[0], A, B, _ptr(wA), _ptr(wB), _ptr(rowcnt), _ptr(out),
                                        _ptr(Y), Y.stride(0), Y.shape[1], _ptr(qpart), self._stream())
        return self._form(rc, "score_gram", out)

    def q_update(self, q: torch.Tensor, qpart: Optional[torch.Tensor] = None, normalize: bool = True,
                 G: Optional[torch.Tensor] = None, q_prev: Optional[torch.Tensor] = None,
                 du2: Optional[torch.Tensor] = None, nparts: Optional[int] = None) -> None:
        """The Y-side update in one launch: q = sum of qpart rows (optional), q /= |q| (optional),
        du2 = (q - q_prev)^T G (q - q_prev) (optional).  tpls.py:100-103."""
        M = q.numel()
        nrows = (nparts or self.n_partials) if qpart is not None else 0
        assert qpart is None or (qpart.is_contiguous() and qpart.numel() >= nrows * M)
        _lib.check(self.lib.cmtfpls_q_update_f64(_ptr(qpart), nrows, M, _ptr(q), int(normalize),
                                                 _ptr(G), _ptr(q_prev), _ptr(du2), self._stream()), "q_update")

    # -- K6: tpls.py:109 ----------------------------------------------------------------------
    def deflate(self, X2, A, B, t, wA, wB) -> torch.Tensor:
        part = self.empty(self.n_partials)
        _lib.check(self._fn("deflate", X2)(_ptr(X2), X2.shape[0], A, B, _ptr(t), _ptr(wA), _ptr(wB), _ptr(part), self._stream()), "deflate")
        return self._close_partials(part)

    def deflate_contract_yq(self, X2, A, B, t, wA, wB, Y: torch.Tensor, q: torch.Tensor, masked: bool,
                            out: torch.Tensor) -> Optional[torch.Tensor]:
        """K6 of one component fused with K1 of the next: X -= t (x) w in place, out = X_new x_0 (Y q); returns
        the sum of squares of X_new (1 double) or None when the shape is outside the fused form."""
        I, P = X2.shape
        ws = self._workspace("deflate_contract", self.lib.cmtfpls_deflate_contract_workspace_bytes(I, P))
        ssq = self.empty(1)
        rc = self._fn("deflate_contract_yq", X2)(_ptr(X2), I, A, B, _ptr(t), _ptr(wA), _ptr(wB), _ptr(Y), Y.stride(0), Y.shape[1],
                                                 _ptr(q), _ptr(out), int(masked), _ptr(ssq), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "deflate_contract_yq", ssq)

    def score_deflate(self, X2, A, B, wA, wB, rowcnt, out) -> Optional[torch.Tensor]:
        """Fused K3+K6; returns None when the row does not fit (caller then uses score + deflate)."""
        part = self.empty(self.n_partials)
        rc = self._fn("score_deflate", X2)(_ptr(X2), X2.shape[0], A, B, _ptr(wA), _ptr(wB), _ptr(rowcnt), _ptr(out), _ptr(part), self._stream())
        if self._form(rc, "score_deflate") is None:
            return None
        return self._close_partials(part)

    # -- K4/K5/K7/K11 small algebra ----------------------------------------------------------
    def gram_tn(self, A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """C = A^T B for 2-D row-major views (unit inner stride) sharing the leading dimension."""
        if A.dim() == 1:
            A = A.unsqueeze(1)
        if B.dim() == 1:
            B = B.unsqueeze(1)
        assert A.stride(1) == 1 and B.stride(1) == 1 and A.shape[0] == B.shape[0]
        a, b = A.shape[1], B.shape[1]
        ws = self._workspace("small", self.lib.cmtfpls_small_workspace_bytes())
        C = out if out is not None else self.empty(a, b)
        assert C.numel() == a * b and C.is_contiguous()
        _lib.check(self.lib.cmtfpls_gram_tn_f64(_ptr(A), A.stride(0), a, _ptr(B), B.stride(0), b, A.shape[0], _ptr(C),
                                                _ptr(ws), ws.numel(), self._stream()), "gram_tn")
        return C

    def rowdot(self, Y: torch.Tensor, q: torch.Tensor, u_out: torch.Tensor, u_old: Optional[torch.Tensor],
               du2: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        ws = self._workspace("small", self.lib.cmtfpls_small_workspace_bytes())
        if u_old is not None and du2 is None:
            du2 = self.empty(1)
        _lib.check(self.lib.cmtfpls_rowdot_f64(_ptr(Y), Y.stride(0), Y.shape[1], Y.shape[0], _ptr(q), _ptr(u_out), _ptr(u_old),
                                               _ptr(du2) if u_old is not None else None,
                                               _ptr(ws), ws.numel(), self._stream()), "rowdot")
        return du2 if u_old is not None else None

    # -- component epilogue / projection fix-up / reconstruction without a host round trip --------
    def normal_solve(self, G: torch.Tensor, g: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """b = argmin |T b - u| from G = T^T T (k x k), g = T^T u: lstsq(T, u, rcond=-1) of tpls.py:110-112."""
        k = G.shape[0]
        assert G.is_contiguous() and G.shape == (k, k) and g.numel() == k
        b = out if out is not None else self.empty(k)
        if k <= 64:
            _lib.check(self.lib.cmtfpls_normal_solve_f64(_ptr(G), _ptr(g), k, _ptr(b), 1, self._stream()), "normal_solve")
        else:                                                   # more than 64 components: the matrix in a workspace
            ws = self._workspace("normal_solve", self.lib.cmtfpls_normal_solve_workspace_bytes(k))
            _lib.check(self.lib.cmtfpls_normal_solve_ws_f64(_ptr(G), _ptr(g), k, _ptr(b), 1, _ptr(ws), ws.numel(), self._stream()),
                       "normal_solve")
        return b

    def unit_upper_solve_rows(self, M: torch.Tensor, U: torch.Tensor, shift: Optional[torch.Tensor] = None,
                              nan_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rows of M (I x R) overwritten by the rows of T solving T (I + triu(U, 1)) = M - 1 shift^T; nan_flag (one int32,
        zeroed by the caller) is set when M holds a NaN."""
        I, R = M.shape
        assert M.stride(1) == 1 and U.is_contiguous() and U.shape == (R, R)
        assert shift is None or (shift.is_contiguous() and shift.numel() == R and shift.dtype == torch.float64)
        assert nan_flag is None or nan_flag.dtype == torch.int32
        _lib.check(self.lib.cmtfpls_unit_upper_solve_rows_f64(_ptr(M), I, M.stride(0), R, _ptr(U), _ptr(shift), _ptr(nan_flag),
                                                              self._stream()), "unit_upper_solve_rows")
        return M

    def kr_gram_row(self, L: torch.Tensor, a: int, g: torch.Tensor, first: bool) -> torch.Tensor:
        """g[:a] (*)= L[:, :a]^T L[:, a]: row a of the loadings' Gram matrix (cmtfpls_kr_gram_row_f64)."""
        assert L.is_contiguous() and g.is_contiguous() and g.numel() >= a
        _lib.check(self.lib.cmtfpls_kr_gram_row_f64(_ptr(L), L.shape[0], L.shape[1], int(a), _ptr(g), int(first), self._stream()), "kr_gram_row")
        return g

    def kr_gram(self, L: torch.Tensor, G: torch.Tensor, first: bool) -> torch.Tensor:
        """G = L^T L (first) or G .*= L^T L: Gram of a Khatri-Rao product, one mode at a time."""
        n, R = L.shape
        assert L.is_contiguous() and G.is_contiguous() and G.numel() == R * R
        _lib.check(self.lib.cmtfpls_kr_gram_f64(_ptr(L), n, R, _ptr(G), int(first), 1.0, self._stream()), "kr_gram")
        return G

    def khatri_rao(self, Am: torch.Tensor, Bm: torch.Tensor) -> torch.Tensor:
        na, R = Am.shape
        nb = Bm.shape[0]
        assert Am.is_contiguous() and Bm.is_contiguous() and Bm.shape[1] == R
        out = self.empty(na * nb, R)
        _lib.check(self.lib.cmtfpls_khatri_rao_f64(_ptr(Am), na, _ptr(Bm), nb, R, _ptr(out), self._stream()), "khatri_rao")
        return out

    def project_rows(self, X2: torch.Tensor, A: int, B: int, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor],
                     out: torch.Tensor, rows: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """out (I, R) = the R sequential masked project-and-deflate steps of every row of the UNCENTRED X2 -- or of the rows
        listed in `rows` (int64 device tensor) only, the others left as they are -- the row kept in registers (one read,
        nothing written); None when the shape is outside that form."""
        I, R = X2.shape[0], WA.shape[1]
        assert WA.is_contiguous() and WB.is_contiguous() and out.stride(1) == 1 and out.shape == (I, R)
        if rows is not None:
            assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.device == self.device
            rc = self._fn("project_rows_idx", X2)(_ptr(X2), _ptr(rows), rows.numel(), A, B, R, _ptr(WA), _ptr(WB), _ptr(mean), _ptr(out),
                                                  out.stride(0), self._stream())
        else:
            rc = self._fn("project_rows", X2)(_ptr(X2), I, A, B, R, _ptr(WA), _ptr(WB), _ptr(mean), _ptr(out), out.stride(0), self._stream())
        return self._form(rc, "project_rows", out)

    def project_rows2(self, X2s, As, Bs, WAs, WBs, means, out: torch.Tensor, rows: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """project_rows for TWO COUPLED blocks (lists of two): the sample's row of both blocks in one workgroup, the score
        of every step the mean of the two masked block scores (cmtf.py:155,206); `rows` as in project_rows; None outside
        that form."""
        I, R = X2s[0].shape[0], WAs[0].shape[1]
        if X2s[0].dtype != X2s[1].dtype or X2s[1].shape[0] != I:
            return None
        assert all(w.is_contiguous() for w in list(WAs) + list(WBs)) and out.stride(1) == 1 and out.shape == (I, R)
        head = (_ptr(X2s[0]), As[0], Bs[0], _ptr(WAs[0]), _ptr(WBs[0]), _ptr(means[0]),
                _ptr(X2s[1]), As[1], Bs[1], _ptr(WAs[1]), _ptr(WBs[1]), _ptr(means[1]))
        if rows is not None:
            assert rows.dtype == torch.int64 and rows.is_contiguous() and rows.device == self.device
            rc = self._fn("project_rows2_idx", X2s[0])(*head, _ptr(rows), rows.numel(), R, _ptr(out), out.stride(0), self._stream())
        else:
            rc = self._fn("project_rows2", X2s[0])(*head, I, R, _ptr(out), out.stride(0), self._stream())
        return self._form(rc, "project_rows2", out)

    def predict_rows(self, S: torch.Tensor, Bm: torch.Tensor, mean: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """out (I, M) = S (I, R) @ Bm (R, M) + mean: the last line of predict (tpls.py:143) on the device-resident scores."""
        I, R = S.shape
        M = Bm.shape[1]
        assert S.stride(1) == 1 and Bm.is_contiguous() and Bm.shape[0] == R
        out = self.empty(I, M)
        rc = self.lib.cmtfpls_predict_rows_f64(_ptr(S), I, S.stride(0), R, _ptr(Bm), M, _ptr(mean), _ptr(out), M, self._stream())
        return self._form(rc, "predict_rows", out)

    def recon(self, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor], out: torch.Tensor) -> Optional[torch.Tensor]:
        """out (I, A*B) = T (WA (.) WB)^T + mean in out's dtype (factors_to_tensor util.py:18-20 + X_mean);
        None when the shape is outside the vector form (caller falls back to the host einsum)."""
        I, R = T.shape
        A, B = WA.shape[0], WB.shape[0]
        assert T.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and out.is_contiguous() and out.numel() == I * A * B
        rc = self._fn("recon", out)(_ptr(T), I, T.stride(0), R, _ptr(WA), _ptr(WB), A, B, _ptr(mean), _ptr(out), self._stream())
        return self._form(rc, "recon", out)

    def recon_r2(self, X2: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """[sum (xhat - x)^2, sum x^2] over the finite entries of x = X2 - mean: calcR2X's two sums (util.py:7-15) against
        the never-materialised reconstruction; None when the shape has no device form."""
        I, P = X2.shape
        R = T.shape[1]
        A, B = WA.shape[0], WB.shape[0]
        assert X2.is_contiguous() and T.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and P == A * B
        ws = self._workspace("recon_r2", self.lib.cmtfpls_recon_r2_workspace_bytes(I, P))
        out = self.empty(2)
        rc = self._fn("recon_r2", X2)(_ptr(X2), _ptr(T), I, T.stride(0), R, _ptr(WA), _ptr(WB), A, B, _ptr(mean), _ptr(out),
                                     _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "recon_r2", out)

    def resid_rows(self, X2: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor],
                   want_cols: bool) -> Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
        """recon_r2's residual kept per row and per column, in one read of X2 (uncentred, storage type): rows (I, 3) =
        [sum e^2, sum x^2, observed entries] per sample and, with want_cols, cols (P, 2) = [sum e^2, sum x^2] per variable,
        x = X2 - mean over its finite entries, e = x - T (WA (.) WB)^T; None when the shape has no device form (R > 16)."""
        I, P = X2.shape
        R = T.shape[1]
        A, B = WA.shape[0], WB.shape[0]
        assert X2.is_contiguous() and T.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and P == A * B
        ws = self._workspace("resid_rows", self.lib.cmtfpls_resid_rows_workspace_bytes(I, P))
        rows = self.empty(I, 3)
        cols = self.empty(P, 2) if want_cols else None
        rc = self._fn("resid_rows", X2)(_ptr(X2), _ptr(T), I, T.stride(0), R, _ptr(WA), _ptr(WB), A, B, _ptr(mean), _ptr(rows),
                                       _ptr(cols), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "resid_rows", (rows, cols))

    def contrib_rows(self, X2: torch.Tensor, T: torch.Tensor, H: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor,
                     mean: Optional[torch.Tensor], rows: Optional[torch.Tensor] = None):
        """Per-mode SPE and T^2 contributions of n samples in one read of their rows of X2 (uncentred, storage type): (speA (n, A),
        speB (n, B), t2A (n, A), t2B (n, B)) with e = x - T (WA (.) WB)^T and d = x * (H (WA (.) WB)^T) over the finite entries of
        x = X2 - mean, e^2 and d summed over the other mode (cmtfpls_contrib_rows_*).  Output row i reads row rows[i] of X2 (int64 on
        the device; None: row i) and rows i of T and H.  A matrix block (A = 1) gets speA = t2A = None.  None when the shape has no
        device form: R > 16, or 2 A (R + 1) doubles beyond the LDS.  No workspace: a workgroup closes both sums of its rows."""
        I, P = X2.shape
        n, R = T.shape
        A, B = WA.shape[0], WB.shape[0]
        assert X2.is_contiguous() and T.stride(1) == 1 and H.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and P == A * B
        assert H.shape == T.shape and (rows is None or (rows.dtype == torch.int64 and rows.is_contiguous() and rows.numel() == n))
        speB, t2B = self.empty(n, B), self.empty(n, B)
        speA, t2A = (self.empty(n, A), self.empty(n, A)) if A > 1 else (None, None)
        rc = self._fn("contrib_rows", X2)(_ptr(X2), I, _ptr(T), T.stride(0), _ptr(H), H.stride(0), R, _ptr(WA), _ptr(WB), A, B, _ptr(mean),
                                         _ptr(rows), n, _ptr(speA), _ptr(speB), _ptr(t2A), _ptr(t2B), self._stream())
        return self._form(rc, "contrib_rows", (speA, speB, t2A, t2B))

    def selectivity_cols(self, X2: torch.Tensor, Tau: torch.Tensor, mean: Optional[torch.Tensor], masked: bool):
        """The target-projection sums of every column in one read of X2 (uncentred, storage type): (a (M, P), d (M, P) or None, s (P,),
        n (P,)) with x = X2 - mean, o = isfinite(x) when masked (else 1): a = sum_i o x tau, d = sum_i o tau^2 (masked only; complete:
        the caller's sum_i tau^2), s = sum_i o x^2, n = sum_i o (cmtfpls_selectivity_cols_*).  Any number of responses: passes of 64
        (masked: 32) inside the entry."""
        I, P = X2.shape
        M = Tau.shape[1]
        assert X2.is_contiguous() and Tau.stride(1) == 1 and Tau.shape[0] == I and Tau.dtype == torch.float64
        assert mean is None or (mean.is_contiguous() and mean.numel() == P and mean.dtype == torch.float64)
        ws = self._workspace("selectivity", self.lib.cmtfpls_selectivity_cols_workspace_bytes(I, P, M))
        a = self.empty(M, P)
        d = self.empty(M, P) if masked else None
        s, n = self.empty(P), self.empty(P)
        _lib.check(self._fn("selectivity_cols", X2)(_ptr(X2), I, P, _ptr(Tau), Tau.stride(0), M, _ptr(mean), int(bool(masked)), _ptr(a),
                                                    _ptr(d), _ptr(s), _ptr(n), _ptr(ws), ws.numel(), self._stream()), "selectivity_cols")
        return a, d, s, n

    def holdout_mask(self, X: torch.Tensor, out: torch.Tensor, fraction: float, seed: int, stream: int, offset: int = 0) -> torch.Tensor:
        """out = X with its held-out entries (the counter rule of include/cmtfpls.h: Philox stream `stream` = 2 + block index keyed by
        `seed`, element index + `offset`) replaced by NaN; X is only read, out is another tensor of X's shape and type.  Returns
        counts (2,) = [entries newly hidden, finite entries left].  One read, one write (cmtfpls_holdout_mask_*)."""
        assert out.is_contiguous() and out.dtype == X.dtype and out.numel() == X.numel() and out.data_ptr() != X.data_ptr()
        n = X.numel()
        ws = self._workspace("holdout_mask", self.lib.cmtfpls_holdout_mask_workspace_bytes(n))
        counts = self.empty(2)
        _lib.check(self._fn("holdout_mask", X)(_ptr(X), _ptr(out), n, float(fraction), int(seed) & (2 ** 64 - 1), int(stream), int(offset),
                                               _ptr(counts), _ptr(ws), ws.numel(), self._stream()), "holdout_mask")
        return counts

    def heldout_resid(self, X2: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor],
                      fraction: float, seed: int, stream: int, offset: int = 0) -> Optional[torch.Tensor]:
        """(R + 2,) = [sum (x - xhat_r)^2 for r = 1..R, sum (x - mean)^2, count] over the held-out finite entries of the ORIGINAL X2
        (uncentred, storage type), xhat_r = mean + the first r components of T (WA (.) WB)^T; the mask is regenerated from the
        counter.  One read (cmtfpls_heldout_resid_*); None when the shape has no device form (R > 16)."""
        I, P = X2.shape
        R = T.shape[1]
        A, B = WA.shape[0], WB.shape[0]
        assert X2.is_contiguous() and T.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and P == A * B
        ws = self._workspace("heldout_resid", self.lib.cmtfpls_heldout_resid_workspace_bytes(I, P, R))
        out = self.empty(R + 2)
        rc = self._fn("heldout_resid", X2)(_ptr(X2), I, A, B, _ptr(T), T.stride(0), R, _ptr(WA), _ptr(WB), _ptr(mean), float(fraction),
                                          int(seed) & (2 ** 64 - 1), int(stream), int(offset), _ptr(out), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "heldout_resid", out)

    def impute(self, X2: torch.Tensor, out: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor,
               mean: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """out = X2 with every non-finite entry replaced by mean + T (WA (.) WB)^T there, rounded once to the storage type; finite
        entries bit for bit.  out may be X2 itself (then only the 16-byte vectors that held a non-finite entry are stored).  Returns
        count (1,) = entries imputed (cmtfpls_impute_*); None when the shape has no device form (R > 16)."""
        I, P = X2.shape
        R = T.shape[1]
        A, B = WA.shape[0], WB.shape[0]
        assert X2.is_contiguous() and out.is_contiguous() and out.dtype == X2.dtype and out.numel() == X2.numel()
        assert T.stride(1) == 1 and WA.is_contiguous() and WB.is_contiguous() and P == A * B
        ws = self._workspace("impute", self.lib.cmtfpls_impute_workspace_bytes(I, P))
        count = self.empty(1)
        rc = self._fn("impute", X2)(_ptr(X2), _ptr(out), I, A, B, _ptr(T), T.stride(0), R, _ptr(WA), _ptr(WB), _ptr(mean), _ptr(count),
                                   _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "impute", count)

    def _loo_folds(self, name: str, fn, head, per_fn, per_args, I: int, M: int, R: int, tol: float, max_iter: int, budget: int,
                   cap: Optional[int] = 512, outs=None) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """The chunked launch of a workgroup-per-fold leave-one-out entry `fn`: head are its arguments before tol (the inputs, their
        column sums and the sizes), per_fn(*per_args) its workspace bytes per fold.  Returns (Ypred (I, M), n_iter (I, R)) -- `outs`
        when given -- or None when the entry declines the shape.  (cap 512: two workgroups' worth of folds per CU is all a launch can
        overlap.)"""
        Ypred, n_iter = outs or (self.empty(I, M), torch.zeros(I, R, dtype=torch.int32, device=self.device))
        if self._chunked_launch(name, lambda f0, nf, ws, nb: fn(*head, float(tol), int(max_iter), f0, nf, _ptr(Ypred), _ptr(n_iter), ws,
                                                                nb, self._stream()),
                                I, lambda: per_fn(*per_args), budget, cap=cap, ws_key="loo") is None:
            return None
        return Ypred, n_iter

    def loo_tpls(self, X2: torch.Tensor, Y: torch.Tensor, A: int, B: int, R: int, tol: float, max_iter: int,
                 max_ws_bytes: Optional[int] = None, forms=("lds", "xcov")) -> Optional[Tuple[torch.Tensor, torch.Tensor, str]]:
        """Leave-one-out predictions of a tPLS model (validate.py:24-33), every fold a workgroup: returns
        (Ypred (I, M), n_iter (I, R), form) or None when the shape is outside both workgroup-per-fold forms.  form:
        "lds" = cmtfpls_loo_tpls_f64 (the fold's vectors in LDS: min(A, B) <= 64), "xcov" = cmtfpls_loo_xcov_f64 (the fold's loop on
        its cross-covariance, Gram squarings on the matrix cores: min(A, B) <= 256).  Folds run in chunks that fit `max_ws_bytes`
        (default: a third of the free HBM) -- the xcov form keeps a centred copy of X per resident fold."""
        I, P = X2.shape
        M = Y.shape[1]
        assert X2.dtype == torch.float64 and Y.dtype == torch.float64 and X2.is_contiguous() and Y.is_contiguous() and P == A * B
        colsum_x, _ = self.colstats(X2)
        colsum_y, _ = self.colstats(Y)
        outs = self.empty(I, M), torch.zeros(I, R, dtype=torch.int32, device=self.device)
        for form, per_fn, fn in (("lds", self.lib.cmtfpls_loo_fold_workspace_bytes, self.lib.cmtfpls_loo_tpls_f64),
                                 ("xcov", self.lib.cmtfpls_loo_xcov_fold_workspace_bytes, self.lib.cmtfpls_loo_xcov_f64)):
            if form not in forms:
                continue
            xcov = form == "xcov"                            # (the lds form: no cap, the 4 GiB budget)
            if self._loo_folds("loo_" + form, fn, (_ptr(X2), _ptr(Y), _ptr(colsum_x), _ptr(colsum_y), I, A, B, M, R), per_fn,
                               (I, A, B, M, R), I, M, R, tol, max_iter, self._ws_budget(max_ws_bytes, xcov),
                               cap=512 if xcov else None, outs=outs) is not None:
                return (*outs, form)
        return None

    def loo_tpls_tensor(self, X2: torch.Tensor, Y: torch.Tensor, A: int, B1: int, B2: int, R: int, tol: float, max_iter: int,
                        max_ws_bytes: Optional[int] = None) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """loo_tpls for X of order 4 (I x A x B1 x B2 as I x A B1 B2): the xcov form with the rank-1 CP of each fold's A x B1 x B2
        cross-covariance inside its workgroup (cmtfpls_loo_xcov_tensor_f64).  Returns (Ypred (I, M), n_iter (I, R)) or None when the
        shape is outside the form.  Folds run in chunks as loo_tpls's xcov form (a centred copy of X per resident fold)."""
        I, P = X2.shape
        M = Y.shape[1]
        assert X2.dtype == torch.float64 and Y.dtype == torch.float64 and X2.is_contiguous() and Y.is_contiguous() and P == A * B1 * B2
        colsum_x, _ = self.colstats(X2)
        colsum_y, _ = self.colstats(Y)
        return self._loo_folds("loo_xcov_tensor", self.lib.cmtfpls_loo_xcov_tensor_f64,
                               (_ptr(X2), _ptr(Y), _ptr(colsum_x), _ptr(colsum_y), I, A, B1, B2, M, R),
                               self.lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes, (I, A, B1, B2, M, R), I, M, R, tol, max_iter,
                               self._ws_budget(max_ws_bytes, True))

    def _loo_coupled(self, name: str, Xs, Y: torch.Tensor, dims, pairs, R: int, tol: float, max_iter: int,
                     max_ws_bytes: Optional[int]) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """loo_ctpls (pairs = ()) and loo_ctpls_tensor (pairs = (the (B1, B2) int array,)): cmtfpls_<name>_f64 on the blocks' description,
        through _loo_folds."""
        nb = len(Xs)
        I, M = Y.shape
        assert nb >= 1 and len(dims) == nb and Y.dtype == torch.float64 and Y.is_contiguous()
        for X2, (_, A, B) in zip(Xs, dims):
            assert X2.dtype == torch.float64 and X2.is_contiguous() and tuple(X2.shape) == (I, A * B)
        colsums = [self.colstats(X2)[0] for X2 in Xs]
        colsum_y, _ = self.colstats(Y)
        blocks = (_lib.LooCoupledBlock * nb)(*[_lib.LooCoupledBlock(_ptr(X2), _ptr(cs), int(o), int(A), int(B))
                                               for X2, cs, (o, A, B) in zip(Xs, colsums, dims)])
        return self._loo_folds("loo_" + name, getattr(self.lib, f"cmtfpls_loo_{name}_f64"),
                               (blocks, nb, *pairs, _ptr(Y), _ptr(colsum_y), I, M, R),
                               getattr(self.lib, f"cmtfpls_loo_{name}_fold_workspace_bytes"), (blocks, nb, *pairs, I, M, R), I, M, R, tol,
                               max_iter, self._ws_budget(max_ws_bytes, True))

    def loo_ctpls(self, Xs, Y: torch.Tensor, dims, R: int, tol: float, max_iter: int,
                  max_ws_bytes: Optional[int] = None) -> Optional[Tuple[torch.Tensor, torch.Tensor, str]]:
        """Leave-one-out predictions of a ctPLS model on complete data (validate.py:24-33 over cmtf.py:85-177), every fold a workgroup
        on the fold's cross-covariances (cmtfpls_loo_xcov_coupled_f64).  Xs: the blocks, each I x P_b float64; dims: (order, A, B) per
        block (order 2: A = 1).  Returns (Ypred (I, M), n_iter (I, R), "xcov_coupled") or None when the shape is outside the form.
        Folds run in chunks as loo_tpls's xcov form (a centred copy of every block per resident fold)."""
        res = self._loo_coupled("xcov_coupled", Xs, Y, dims, (), R, tol, max_iter, max_ws_bytes)
        return None if res is None else (*res, "xcov_coupled")

    def loo_ctpls_tensor(self, Xs, Y: torch.Tensor, dims, tensor, R: int, tol: float, max_iter: int,
                         max_ws_bytes: Optional[int] = None) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """loo_ctpls for a ctPLS with blocks of order 4 (cmtfpls_loo_xcov_coupled_tensor_f64): a block I x A x B1 x B2 is given as
        I x A B1 B2 with dims (4, A, B1 B2) and tensor (B1, B2); a block of order 2 or 3 has tensor (0, 0).  The extraction of a tensor
        block is the rank-1 CP of its cross-covariance inside the fold's workgroup.  Returns (Ypred (I, M), n_iter (I, R)) or None
        when the shape is outside the form.  Folds run in chunks as loo_ctpls's."""
        assert len(tensor) == len(Xs)
        return self._loo_coupled("xcov_coupled_tensor", Xs, Y, dims, (_int_pairs(tensor),), R, tol, max_iter, max_ws_bytes)

    def _masked_outputs(self, n: int, I: int, M: int, R: int, per_model: bool, factors) -> dict:
        """The zeroed outputs of a masked cross-validation entry over n folds or models: Ypred (R, I, M), per_model: (n, R, I, M),
        n_iter (n, R), status (n), info (n, 2) and a (n, *shape) tensor per entry of `factors` (name -> shape)."""
        out = {"Ypred": self.zeros(*((n,) if per_model else ()), R, I, M), "n_iter": torch.zeros(n, R, dtype=torch.int32, device=self.device),
               "status": torch.zeros(n, dtype=torch.int32, device=self.device),
               "info": torch.zeros(n, 2, dtype=torch.int32, device=self.device)}
        out.update({k: self.zeros(n, *shape) for k, shape in factors.items()})
        return out

    def _masked_launch(self, name: str, args, out: dict, factors, n: int, per_fn, max_ws_bytes: Optional[int], extra: int = 0):
        """The chunked launch of cmtfpls_<name>_f64(*args, first, count, Ypred, the outputs named in `factors` (NULL where `out` has
        none), n_iter, status, info, ws, ws_bytes, stream) over n folds or models: `out` with its "launches", or None when the entry
        declines the shape."""
        fn = getattr(self.lib, f"cmtfpls_{name}_f64")
        outs = tuple(_ptr(out.get(k)) for k in ("Ypred", *factors, "n_iter", "status", "info"))
        out["launches"] = self._chunked_launch(name, lambda i0, cnt, ws, nb: fn(*args, i0, cnt, *outs, ws, nb, self._stream()), n, per_fn,
                                               self._ws_budget(max_ws_bytes), extra=extra)
        return out if out["launches"] is not None else None

    def _cv_masked_folds(self, X2: torch.Tensor, Y: torch.Tensor, fold_of: torch.Tensor, K: int, A: int, B: int, tensor, R: int,
                         tol: float, max_iter: int, max_ws_bytes: Optional[int]):
        """cv_masked (tensor None) and cv_masked_tensor (tensor = (B1, B2), B = B1 B2): cmtfpls_cv_masked[_tensor]_f64 through
        _masked_launch.  Returns (Ypred, n_iter, status, info, launches) or None when the entry declines the shape."""
        name, trail = ("cv_masked_tensor", tuple(tensor)) if tensor else ("cv_masked", (B,))
        I, P = X2.shape
        M = Y.shape[1]
        assert X2.dtype == torch.float64 and Y.dtype == torch.float64 and X2.is_contiguous() and Y.is_contiguous() and P == A * B
        assert fold_of.dtype == torch.int32 and fold_of.is_contiguous() and fold_of.numel() == I
        colsum_x, colcnt_x = self.colstats(X2)
        colsum_y, _ = self.colstats(Y)
        args = (_ptr(X2), _ptr(Y), _ptr(fold_of), int(K), _ptr(colsum_x), _ptr(colcnt_x), _ptr(colsum_y), I, A, *trail, M, R, float(tol),
                int(max_iter))
        per_fn = getattr(self.lib, f"cmtfpls_{name}_fold_workspace_bytes")
        out = self._masked_launch(name, args, self._masked_outputs(K, I, M, R, False, {}), (), K, lambda: per_fn(I, A, *trail, M, R),
                                  max_ws_bytes)
        return None if out is None else (out["Ypred"], out["n_iter"], out["status"], out["info"], out["launches"])

    def cv_masked(self, X2: torch.Tensor, Y: torch.Tensor, fold_of: torch.Tensor, K: int, A: int, B: int, R: int, tol: float,
                  max_iter: int, max_ws_bytes: Optional[int] = None
                  ) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]:
        """Cross-validation refits of a tPLS on X2 with missing values (NaN), a workgroup per fold (cmtfpls_cv_masked_f64): returns
        (Ypred (R, I, M): [r - 1, i] = row i predicted by its fold's model with r components, n_iter (K, R), status (K), info (K, 2):
        whether the fold's training rows / held-out batch took the masked arithmetic), or None when the shape is outside the form.
        fold_of: (I,) int32 fold ids 0..K-1 (leave-one-out: arange(I), K = I).  Folds run in chunks whose workspace fits
        `max_ws_bytes` (default 4 GiB); the workspace is allocated per call and released with it."""
        out = self._cv_masked_folds(X2, Y, fold_of, K, A, B, None, R, tol, max_iter, max_ws_bytes)
        return None if out is None else out[:4]

    def cv_masked_tensor(self, X2: torch.Tensor, Y: torch.Tensor, fold_of: torch.Tensor, K: int, A: int, B1: int, B2: int, R: int,
                         tol: float, max_iter: int, max_ws_bytes: Optional[int] = None
                         ) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, int]]:
        """cv_masked for X of order 4 (I x A x B1 x B2 as I x A B1 B2, NaN = missing): the rank-1 CP of each fold's A x B1 x B2
        contraction inside its workgroup (cmtfpls_cv_masked_tensor_f64).  Returns cv_masked's (Ypred, n_iter, status, info) and the
        number of launches, or None when the shape is outside the form."""
        return self._cv_masked_folds(X2, Y, fold_of, K, A, B1 * B2, (B1, B2), R, tol, max_iter, max_ws_bytes)

    def _cv_masked_models(self, X2: torch.Tensor, Y: torch.Tensor, counts: torch.Tensor, yrow: Optional[torch.Tensor], A: int, B: int,
                          tensor, R: int, tol: float, max_iter: int, factors: bool, max_ws_bytes: Optional[int]) -> Optional[dict]:
        """cv_masked_models (tensor None) and cv_masked_tensor_models (tensor = (B1, B2), B = B1 B2): cmtfpls_cv_masked[_tensor]_models_f64
        through _masked_launch, the trailing loadings Wb, or Wk and Wl."""
        name, trail = ("cv_masked_tensor", tuple(tensor)) if tensor else ("cv_masked", (B,))
        I, P = X2.shape
        M = Y.shape[1]
        nm = counts.shape[0]
        assert X2.dtype == torch.float64 and Y.dtype == torch.float64 and X2.is_contiguous() and Y.is_contiguous() and P == A * B
        assert counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (nm, I) and nm > 0
        assert yrow is None or (yrow.dtype == torch.int32 and yrow.is_contiguous() and tuple(yrow.shape) == (nm, I))
        trailing = {"Wk": (R, trail[0]), "Wl": (R, trail[1])} if tensor else {"Wb": (R, B)}
        shapes = {"Wa": (R, A), **trailing, "coef": (R, R), "Q": (R, M)}
        args = (_ptr(X2), _ptr(Y), _ptr(counts), _ptr(yrow), nm, I, A, *trail, M, R, float(tol), int(max_iter))
        per_fn = getattr(self.lib, f"cmtfpls_{name}_model_workspace_bytes")
        return self._masked_launch(name + "_models", args, self._masked_outputs(nm, I, M, R, True, shapes if factors else {}), shapes, nm,
                                   lambda: per_fn(I, A, *trail, M, R), max_ws_bytes, extra=R * I * M * 8)

    def cv_masked_models(self, X2: torch.Tensor, Y: torch.Tensor, counts: torch.Tensor, yrow: Optional[torch.Tensor], A: int, B: int,
                         R: int, tol: float, max_iter: int, factors: bool = False, max_ws_bytes: Optional[int] = None
                         ) -> Optional[dict]:
        """Refits of a tPLS on X2 with missing values (NaN) on count-weighted rows, a workgroup per model
        (cmtfpls_cv_masked_models_f64): model m trains on counts[m, r] copies of X row r paired with Y row yrow[m, r] and predicts
        its rows with count 0.  counts: (n, I) int32; yrow: (n, I) int32 or None (identity).  Returns a dict of device tensors --
        Ypred (n, R, I, M) (zero where the model trained), n_iter (n, R), status (n), info (n, 2) and with `factors` Wa (n, R, A),
        Wb (n, R, B), coef (n, R, R), Q (n, R, M) -- or None when the shape is outside the form.  Models run in chunks whose
        workspace and Ypred rows fit `max_ws_bytes` (default 4 GiB); the workspace is allocated per call and released with it."""
        return self._cv_masked_models(X2, Y, counts, yrow, A, B, None, R, tol, max_iter, factors, max_ws_bytes)

    def cv_masked_tensor_models(self, X2: torch.Tensor, Y: torch.Tensor, counts: torch.Tensor, yrow: Optional[torch.Tensor], A: int,
                                B1: int, B2: int, R: int, tol: float, max_iter: int, factors: bool = False,
                                max_ws_bytes: Optional[int] = None) -> Optional[dict]:
        """cv_masked_models for X of order 4 (I x A x B1 x B2 as I x A B1 B2, NaN = missing; cmtfpls_cv_masked_tensor_models_f64).
        Returns cv_masked_models' dict, with `factors` Wa (n, R, A), Wk (n, R, B1), Wl (n, R, B2), coef and Q, or None when the
        shape is outside the form."""
        return self._cv_masked_models(X2, Y, counts, yrow, A, B1 * B2, (B1, B2), R, tol, max_iter, factors, max_ws_bytes)

    def _cv_masked_coupled(self, name: str, X2s, dims, tensor, pairs, Y: torch.Tensor, counts: torch.Tensor,
                           yrow: Optional[torch.Tensor], R: int, tol: float, max_iter: int, factors: bool,
                           max_ws_bytes: Optional[int]) -> Optional[dict]:
        """cv_masked_coupled (pairs = (), tensor (0, 0) per block) and cv_masked_coupled_tensor (pairs = (the (B1, B2) int array,)):
        cmtfpls_<name>_f64 on the blocks' description through _masked_launch, then with `factors` every block's slice of the
        loadings (Wk, Wl only with pairs)."""
        nb = len(X2s)
        I = X2s[0].shape[0]
        M = Y.shape[1]
        nm = counts.shape[0]
        assert nb >= 1 and len(dims) == nb and len(tensor) == nb and Y.dtype == torch.float64 and Y.is_contiguous() and Y.shape[0] == I
        for X2, (_, A, B) in zip(X2s, dims):
            assert X2.dtype == torch.float64 and X2.is_contiguous() and tuple(X2.shape) == (I, A * B)
        assert counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (nm, I) and nm > 0
        assert yrow is None or (yrow.dtype == torch.int32 and yrow.is_contiguous() and tuple(yrow.shape) == (nm, I))
        blocks = (_lib.CvCoupledBlock * nb)(*[_lib.CvCoupledBlock(_ptr(X2), int(o), int(A), int(B)) for X2, (o, A, B) in zip(X2s, dims)])
        sumA, sumB = sum(A for _, A, _ in dims), sum(B for _, _, B in dims)
        sumK, sumL = sum(B1 for B1, B2 in tensor if B2 > 0), sum(B2 for _, B2 in tensor)
        modes = {"Wk": (R * sumK,), "Wl": (R * sumL,)} if pairs else {}
        shapes = {"Wa": (R * sumA,), "Wb": (R * sumB,), **modes, "coef": (R, R), "Q": (R, M)}
        args = (blocks, nb, *pairs, _ptr(Y), _ptr(counts), _ptr(yrow), nm, I, M, R, float(tol), int(max_iter))
        per_fn = getattr(self.lib, f"cmtfpls_{name}_workspace_bytes")
        out = self._masked_launch(name, args, self._masked_outputs(nm, I, M, R, True, shapes if factors else {}), shapes, nm,
                                  lambda: per_fn(blocks, nb, *pairs, I, M, R), max_ws_bytes, extra=R * I * M * 8)
        def per_block(key, widths):                      # block b's R x n_b at R * (n_0 + .. + n_(b-1)); None for a width of 0
            cut, o = [], 0
            for n in widths:
                cut.append(out[key][:, R * o:R * (o + n)].reshape(nm, R, n) if n else None)
                o += n
            return cut

        if out is not None and factors:
            out["Wa"], out["Wb"] = per_block("Wa", [A for _, A, _ in dims]), per_block("Wb", [B for _, _, B in dims])
            if pairs:                                    # a block of order 2 or 3 has no mode loadings
                out["Wk"] = per_block("Wk", [B1 if B2 > 0 else 0 for B1, B2 in tensor])
                out["Wl"] = per_block("Wl", [B2 for _, B2 in tensor])
        return out

    def cv_masked_coupled(self, X2s, dims, Y: torch.Tensor, counts: torch.Tensor, yrow: Optional[torch.Tensor], R: int, tol: float,
                          max_iter: int, factors: bool = False, max_ws_bytes: Optional[int] = None) -> Optional[dict]:
        """Refits of a ctPLS whose blocks X2s (each I x P_b, NaN = missing) have missing values on count-weighted rows, a workgroup
        per model (cmtfpls_cv_masked_coupled_f64): model m trains on counts[m, r] copies of row r of every block paired with Y row
        yrow[m, r] and predicts its rows with count 0.  dims: (order, A, B) per block; counts: (n, I) int32; yrow: (n, I) int32 or
        None (identity).  Returns a dict of device tensors -- Ypred (n, R, I, M) (zero where the model trained), n_iter (n, R),
        status (n), info (n, 2) (bit masks over the blocks) and with `factors` Wa, Wb (lists: per block (n, R, A_b) / (n, R, B_b)),
        coef (n, R, R), Q (n, R, M) -- or None when the shape is outside the form.  Models run in chunks whose workspace and Ypred
        rows fit `max_ws_bytes` (default 4 GiB); the workspace is allocated per call and released with it."""
        return self._cv_masked_coupled("cv_masked_coupled", X2s, dims, [(0, 0)] * len(X2s), (), Y, counts, yrow, R, tol, max_iter,
                                       factors, max_ws_bytes)

    def cv_masked_coupled_tensor(self, X2s, dims, tensor, Y: torch.Tensor, counts: torch.Tensor, yrow: Optional[torch.Tensor], R: int,
                                 tol: float, max_iter: int, factors: bool = False, max_ws_bytes: Optional[int] = None) -> Optional[dict]:
        """cv_masked_coupled for a ctPLS with blocks of order 4 (cmtfpls_cv_masked_coupled_tensor_f64): a block I x A x B1 x B2 is
        given as I x A B1 B2 with dims (4, A, B1 B2) and tensor (B1, B2); a block of order 2 or 3 has tensor (0, 0).  The loading of a
        tensor block is the rank-1 CP of its contraction inside the model's workgroup.  Returns cv_masked_coupled's dict, with
        `factors` also Wk, Wl (lists: per block (n, R, B1_b) / (n, R, B2_b), None for a block of order 2 or 3; Wb of a tensor block is
        wK (x) wL), or None when the shape is outside the form.  Models run in chunks as cv_masked_coupled's."""
        return self._cv_masked_coupled("cv_masked_coupled_tensor", X2s, dims, tensor, (_int_pairs(tensor),), Y, counts, yrow, R, tol,
                                       max_iter, factors, max_ws_bytes)

    # -- K-fold cross-validation (validate.kfold_predictions, kfold.py): every fold from the same reads of X ----------------
    def kfold_xcov(self, X2: torch.Tensor, A: int, B: int, Y: torch.Tensor, order: torch.Tensor, fold_off: torch.Tensor, K: int,
                   ydev: torch.Tensor, S: torch.Tensor, mean: torch.Tensor) -> Optional[torch.Tensor]:
        """Every fold's training cross-covariance S[k] (K x M x P) and training means (K x P) from ONE read of the uncentred X2
        (cmtfpls_kfold_xcov_*); returns the column sums / sums of squares of all rows (2 P), or None when the shape is outside
        the device form (a 16-bit X2 on a library without the 16-bit entries included).  The partial-sum workspace is local to
        the call."""
        I, P = X2.shape
        M = Y.shape[1]
        fn = self._read_fn("kfold_xcov", X2)
        if fn is None:
            return None
        assert Y.dtype == torch.float64 and Y.is_contiguous() and order.dtype == torch.int32 and fold_off.dtype == torch.int32 and P == A * B
        ws = _scratch(self.lib.cmtfpls_kfold_xcov_workspace_bytes(I, P, M, K), self.device)
        stats = self.empty(2 * P)
        rc = fn(_ptr(X2), I, A, B, _ptr(Y), M, _ptr(order), _ptr(fold_off), K, _ptr(ydev), _ptr(S), _ptr(mean),
                                        _ptr(stats), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_xcov", stats)

    def kfold_inner(self, state, a: int, tol: float, max_iter: int, ws: torch.Tensor) -> Optional[bool]:
        """Component a's inner loop for every fold, a workgroup per fold (cmtfpls_kfold_inner_f64); `state` is a
        _lib.KfoldState, `ws` at least kfold_inner_workspace_bytes.  None when the shape is outside the device form."""
        rc = self.lib.cmtfpls_kfold_inner_f64(ctypes.byref(state), int(a), float(tol), int(max_iter), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_inner")

    def kfold_inner_workspace_bytes(self, A: int, B: int, K: int) -> int:
        return int(self.lib.cmtfpls_kfold_inner_workspace_bytes(A, B, K))

    def kfold_inner_tensor(self, state, B1: int, B2: int, a: int, tol: float, max_iter: int, ws: torch.Tensor,
                           model_fold: Optional[torch.Tensor] = None, groups: int = 1, Wk: Optional[torch.Tensor] = None,
                           Wl: Optional[torch.Tensor] = None) -> Optional[bool]:
        """kfold_inner (model_fold: kfold_inner_grouped) for X of order 4, I x A x B1 x B2 with state.B = B1 * B2: the rank-1 CP of
        each fold's A x B1 x B2 cross-covariance inside its workgroup (cmtfpls_kfold_inner_tensor_f64).  Wk (K x R x B1) and Wl
        (K x R x B2) receive component a's mode loadings; `ws` at least kfold_inner_tensor_workspace_bytes.  None when the shape is
        outside the device form."""
        assert model_fold is None or (model_fold.dtype == torch.int32 and model_fold.numel() == state.K)
        rc = self.lib.cmtfpls_kfold_inner_tensor_f64(ctypes.byref(state), _ptr(model_fold), int(groups), int(B1), int(B2), int(a),
                                                     float(tol), int(max_iter), _ptr(Wk), _ptr(Wl), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_inner_tensor")

    def kfold_inner_tensor_workspace_bytes(self, A: int, B1: int, B2: int, K: int) -> int:
        return int(self.lib.cmtfpls_kfold_inner_tensor_workspace_bytes(A, B1, B2, K))

    def kfold_row_tiles(self, I: int) -> Tuple[int, int]:
        """(row tiles of the K-fold epilogue's grid, doubles of partial sums per tile)."""
        return int(self.lib.cmtfpls_kfold_row_tiles(I)), int(self.lib.cmtfpls_kfold_part_stride())

    def kfold_epilogue(self, state, stage: int, a: int, src: Optional[torch.Tensor]) -> Optional[bool]:
        """Stage 0: every fold's Gy; 1: component a's epilogue from the MTTKRP scores (I x K); 2: the down-date of S from the
        contraction (K x P) -- cmtfpls_kfold_epilogue_f64.  None when the shape is outside the device form."""
        rc = self.lib.cmtfpls_kfold_epilogue_f64(ctypes.byref(state), int(stage), int(a), _ptr(src), self._stream())
        return self._form(rc, "kfold_epilogue")

    def kfold_inner_coupled(self, views, a: int, tol: float, max_iter: int, ws: torch.Tensor) -> Optional[bool]:
        """Component a's inner loop for every fold of a coupled model, a workgroup per fold going through the blocks
        (cmtfpls_kfold_inner_coupled_f64); `views` is a ctypes array of _lib.KfoldState, one per block, `ws` at least
        kfold_inner_coupled_workspace_bytes(views).  None when a block or the LDS is outside the device form."""
        rc = self.lib.cmtfpls_kfold_inner_coupled_f64(views, len(views), int(a), float(tol), int(max_iter), _ptr(ws), ws.numel(),
                                                      self._stream())
        return self._form(rc, "kfold_inner_coupled")

    def kfold_inner_coupled_workspace_bytes(self, views) -> int:
        return int(self.lib.cmtfpls_kfold_inner_coupled_workspace_bytes(views, len(views)))

    def kfold_inner_coupled_tensor(self, views, dims, a: int, tol: float, max_iter: int, ws: torch.Tensor,
                                   model_fold: Optional[torch.Tensor] = None, groups: int = 1, Wk: Optional[torch.Tensor] = None,
                                   Wl: Optional[torch.Tensor] = None) -> Optional[bool]:
        """kfold_inner_coupled (model_fold: kfold_inner_coupled_grouped) for a coupled model with blocks of order 4
        (cmtfpls_kfold_inner_coupled_tensor_f64).  dims: (B1, B2) per block, (0, 0) for a matrix block; a tensor block's view has
        B = B1 * B2 and its extraction is the rank-1 CP inside the fold's workgroup.  Wk / Wl receive component a's mode loadings,
        the tensor blocks' K x R x B1 (B2) slices one after another in block order; `ws` at least
        kfold_inner_coupled_tensor_workspace_bytes(views, dims).  None when a block or the LDS is outside the device form."""
        assert len(dims) == len(views) and (model_fold is None or (model_fold.dtype == torch.int32 and model_fold.numel() == views[0].K))
        rc = self.lib.cmtfpls_kfold_inner_coupled_tensor_f64(views, len(views), _int_pairs(dims), _ptr(model_fold), int(groups), int(a),
                                                             float(tol), int(max_iter), _ptr(Wk), _ptr(Wl), _ptr(ws), ws.numel(),
                                                             self._stream())
        return self._form(rc, "kfold_inner_coupled_tensor")

    def kfold_inner_coupled_tensor_workspace_bytes(self, views, dims) -> int:
        return int(self.lib.cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(views, len(views), _int_pairs(dims)))

    def kfold_combine_scores(self, sc: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out = the average of sc's nb leading slices (nb x I x K), added in block order (cmtfpls_kfold_combine_scores_f64)."""
        assert sc.is_contiguous() and out.is_contiguous() and sc[0].numel() == out.numel()
        _lib.check(self.lib.cmtfpls_kfold_combine_scores_f64(_ptr(sc), sc.shape[0], out.numel(), _ptr(out), self._stream()),
                   "kfold_combine_scores")
        return out

    # -- response-permutation test of K-fold Q2Y (validate.permutation_test_q2y, permutation.py): G permutations x K folds per pass --
    def kfold_wide_xcov(self, X2: torch.Tensor, A: int, B: int, Y: torch.Tensor, order: torch.Tensor, fold_off: torch.Tensor, K: int,
                        ydev: torch.Tensor, S: torch.Tensor, mean: torch.Tensor) -> Optional[torch.Tensor]:
        """kfold_xcov for a wide centred Y' (I x W, W <= 1024: G permuted responses side by side) on the f64 matrix cores
        (cmtfpls_kfold_wide_xcov_*): S (K x W x P), the folds' training means (K x P) and, returned, the column sums / sums of
        squares of all rows (2 P); None when the shape is outside the device form.  The partial-sum workspace is local to the call."""
        I, P = X2.shape
        W = Y.shape[1]
        fn = self._read_fn("kfold_wide_xcov", X2)
        if fn is None:
            return None
        assert Y.dtype == torch.float64 and Y.is_contiguous() and ydev.is_contiguous() and S.is_contiguous() and P == A * B
        assert order.dtype == torch.int32 and fold_off.dtype == torch.int32 and S.numel() == K * W * P and mean.numel() == K * P
        ws = _scratch(self.lib.cmtfpls_kfold_wide_xcov_workspace_bytes(I, P, W, K), self.device)
        stats = self.empty(2 * P)
        rc = fn(_ptr(X2), I, A, B, _ptr(Y), W, _ptr(order), _ptr(fold_off), K, _ptr(ydev), _ptr(S),
                                             _ptr(mean), _ptr(stats), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_wide_xcov", stats)

    def kfold_inner_grouped(self, state, model_fold: torch.Tensor, groups: int, a: int, tol: float, max_iter: int,
                            ws: torch.Tensor) -> Optional[bool]:
        """kfold_inner for state.K models in `groups` groups, model m holding out fold model_fold[m] (cmtfpls_kfold_inner_grouped_f64)."""
        assert model_fold.dtype == torch.int32 and model_fold.numel() == state.K
        rc = self.lib.cmtfpls_kfold_inner_grouped_f64(ctypes.byref(state), _ptr(model_fold), int(groups), int(a), float(tol), int(max_iter),
                                                      _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_inner_grouped")

    def kfold_epilogue_grouped(self, state, model_fold: torch.Tensor, groups: int, stage: int, a: int,
                               src: Optional[torch.Tensor]) -> Optional[bool]:
        """kfold_epilogue for state.K models in `groups` groups (cmtfpls_kfold_epilogue_grouped_f64); held-out scores of group
        m % groups go to that group's I x R slice of Tout."""
        assert model_fold.dtype == torch.int32 and model_fold.numel() == state.K
        rc = self.lib.cmtfpls_kfold_epilogue_grouped_f64(ctypes.byref(state), _ptr(model_fold), int(groups), int(stage), int(a), _ptr(src),
                                                         self._stream())
        return self._form(rc, "kfold_epilogue_grouped")

    def kfold_inner_coupled_grouped(self, views, model_fold: torch.Tensor, groups: int, a: int, tol: float, max_iter: int,
                                    ws: torch.Tensor) -> Optional[bool]:
        """kfold_inner_coupled for views[0].K models in `groups` groups, model m holding out fold model_fold[m]: every view's mean is
        per fold (cmtfpls_kfold_inner_coupled_grouped_f64).  None when a block or the LDS is outside the device form."""
        assert model_fold.dtype == torch.int32 and model_fold.numel() == views[0].K
        rc = self.lib.cmtfpls_kfold_inner_coupled_grouped_f64(views, len(views), _ptr(model_fold), int(groups), int(a), float(tol),
                                                              int(max_iter), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "kfold_inner_coupled_grouped")

    # -- repeated K-fold Q2Y (validate.get_q2y_repeated_kfold, repeated.py): G shuffled splits x K folds per pass ----------------
    def kfold_epilogue_splits(self, state, splits: int, stage: int, a: int, src: Optional[torch.Tensor]) -> Optional[bool]:
        """kfold_epilogue for state.K models in `splits` split-major splits (cmtfpls_kfold_epilogue_splits_f64): fold_of is
        splits x I, and the held-out scores of split m // (K / splits) go to that split's I x R slice of Tout."""
        rc = self.lib.cmtfpls_kfold_epilogue_splits_f64(ctypes.byref(state), int(splits), int(stage), int(a), _ptr(src), self._stream())
        return self._form(rc, "kfold_epilogue_splits")

    # -- bootstrap of the factors (validate.bootstrap_factors, bootstrap.py): n weighted resamples per pass ------------------
    def kfold_weighted_xcov(self, X2: torch.Tensor, A: int, B: int, Y: torch.Tensor, n: int, M: int, S: torch.Tensor,
                            mean: torch.Tensor) -> Optional[torch.Tensor]:
        """Every resample's cross-covariance S (n x M x P) and means (n x P) from ONE read of the uncentred X2 on the f64 matrix
        cores (cmtfpls_kfold_weighted_xcov_*); Y = [c_1 * (Y - nu_1) .. c_n * (Y - nu_n) | c_1 .. c_n] (I x n (M + 1)).  Returns
        the column sums / sums of squares of all rows (2 P), or None when the shape is outside the device form.  The partial-sum
        workspace is local to the call."""
        I, P = X2.shape
        fn = self._read_fn("kfold_weighted_xcov", X2)
        if fn is None:
            return None
        assert Y.dtype == torch.float64 and Y.is_contiguous() and Y.shape == (I, n * (M + 1)) and P == A * B
        assert S.is_contiguous() and S.numel() == n * M * P and mean.is_contiguous() and mean.numel() == n * P
        ws = _scratch(self.lib.cmtfpls_kfold_weighted_xcov_workspace_bytes(I, P, n, M), self.device)
        stats = self.empty(2 * P)
        rc = fn(_ptr(X2), I, A, B, _ptr(Y), n, M, _ptr(S), _ptr(mean), _ptr(stats), _ptr(ws),
                                                 ws.numel(), self._stream())
        return self._form(rc, "kfold_weighted_xcov", stats)

    def kfold_epilogue_weighted(self, state, stage: int, a: int, src: Optional[torch.Tensor]) -> Optional[bool]:
        """kfold_epilogue for state.K weighted models (cmtfpls_kfold_epilogue_weighted_f64): fold_of is the n x I row counts,
        every training-row sum is weighted by them; the rows with count 0 keep their projection in T."""
        rc = self.lib.cmtfpls_kfold_epilogue_weighted_f64(ctypes.byref(state), int(stage), int(a), _ptr(src), self._stream())
        return self._form(rc, "kfold_epilogue_weighted")

    def press_rows(self, T: torch.Tensor, coef: torch.Tensor, Q: torch.Tensor, nu: torch.Tensor, Y: torch.Tensor, ev: torch.Tensor,
                   pred: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """press (n, R): model j's squared prediction errors with r = 1..R components, summed over the rows with ev[j, i] > 0
        (cmtfpls_press_rows_f64): pred_r = nu[j] + sum_{c < r} (T[j, i] @ coef[j])_c Q[j, c] against Y[i].  T (n, I, R), coef
        (n, R, R) upper triangular, Q (n, R, M), nu (n, M), Y (I, M), ev (n, I) int32; where ev == 2 the r-component prediction
        goes to pred[r - 1, i] (pred (R, I, M), optional).  None when R or M is outside the kernel (64 each)."""
        n, I, R = T.shape
        M = Y.shape[1]
        for t, shape in ((T, (n, I, R)), (coef, (n, R, R)), (Q, (n, R, M)), (nu, (n, M)), (Y, (I, M))):
            assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape and t.device == self.device
        assert ev.dtype == torch.int32 and ev.is_contiguous() and tuple(ev.shape) == (n, I) and ev.device == self.device
        assert pred is None or (pred.dtype == torch.float64 and pred.is_contiguous() and tuple(pred.shape) == (R, I, M)
                                and pred.device == self.device)
        ws = self._workspace("press_rows", self.lib.cmtfpls_press_rows_workspace_bytes(n, I, R, M))
        press = self.empty(n, R)
        rc = self.lib.cmtfpls_press_rows_f64(_ptr(T), _ptr(coef), _ptr(Q), _ptr(nu), _ptr(Y), _ptr(ev), n, I, R, M, _ptr(press),
                                             _ptr(pred), _ptr(ws), ws.numel(), self._stream())
        return self._form(rc, "press_rows", press)

    def fit_small(self, X2: torch.Tensor, Y: torch.Tensor, A: int, B: int, R: int, tol: float, max_iter: int):
        """The complete tPLS.fit of a small float64 problem without missing values in ONE launch (cmtfpls_fit_small_f64):
        returns a dict of device tensors (T, U, WA, WB, Q, x_mean, y_mean) and host arrays (coef, ssq, n_iter), or None
        when the shape is outside the one-workgroup form or the input holds a non-finite value (nothing usable written)."""
        I, P = X2.shape
        M = Y.shape[1]
        if X2.dtype != torch.float64 or Y.dtype != torch.float64 or not (X2.is_contiguous() and Y.is_contiguous()) or I >= 2 ** 31 or P != A * B:
            return None
        nbytes = self.lib.cmtfpls_fit_small_workspace_bytes(I, A, B, M)
        T, U = self.empty(I, R), self.empty(I, R)
        WA, WB, Q = self.empty(A, R), self.empty(B, R), self.empty(M, R)
        small = self.empty(R * R + 2 * (R + 1))                      # coef | ssq: one device -> host copy
        xm, ym = self.empty(P), self.empty(M)
        ints = torch.zeros(R + 1, dtype=torch.int32, device=self.device)    # n_iter | flag
        ws = self._workspace("fit_small", max(nbytes, 256))
        rc = self.lib.cmtfpls_fit_small_f64(_ptr(X2), _ptr(Y), I, A, B, M, R, float(tol), int(max_iter), _ptr(T), _ptr(U), _ptr(WA), _ptr(WB),
                                            _ptr(Q), _ptr(small), small[R * R:].data_ptr(), _ptr(xm), _ptr(ym), _ptr(ints),
                                            ints[R:].data_ptr(), _ptr(ws), ws.numel(), self._stream())
        if self._form(rc, "fit_small") is None:
            return None
        ih = ints.cpu().numpy()
        if ih[R] != 0:
            return None                                              # a NaN / inf somewhere: the regular (masked) engine takes it
        sh = small.cpu().numpy()
        return {"T": T, "U": U, "WA": WA, "WB": WB, "Q": Q, "x_mean": xm, "y_mean": ym, "coef": sh[:R * R].reshape(R, R).copy(),
                "ssq": sh[R * R:].reshape(R + 1, 2).copy(), "n_iter": [int(v) for v in ih[:R]]}

    def add_noise(self, X: torch.Tensor, sigma: float, seed: int, offset: int = 0, nan_fraction: float = 0.0) -> torch.Tensor:
        """X += sigma * N(0,1) in place from the counter-based generator (element e of X is global element offset + e
        of the stream keyed by seed), then an i.i.d. NaN mask of density nan_fraction (synthetic.py:71,74)."""
        assert X.is_contiguous() and X.device == self.device
        _lib.check(self._fn("add_noise", X)(_ptr(X), X.numel(), float(sigma), int(seed) & (2 ** 64 - 1), int(offset), float(nan_fraction),
                                            self._stream()), "add_noise")
        return X

    def scores_mean(self, Ts: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        nb, I = Ts.shape
        _lib.check(self.lib.cmtfpls_scores_mean_f64(_ptr(Ts), nb, I, _ptr(out), self._stream()), "scores_mean")
        return out

    def y_deflate(self, Y: torch.Tensor, T: torch.Tensor, ncols: int, b: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
        ws = self._workspace("small", self.lib.cmtfpls_small_workspace_bytes())
        ssq = self.empty(1)
        _lib.check(self.lib.cmtfpls_y_deflate_f64(_ptr(Y), Y.stride(0), Y.shape[1], Y.shape[0], _ptr(T), T.stride(0), ncols, _ptr(b), _ptr(q),
                                                  _ptr(ssq), _ptr(ws), ws.numel(), self._stream()), "y_deflate")
        return ssq
