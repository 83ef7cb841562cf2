"""Workspaces and outputs at their stated size, poisoned and guarded (tests/test_gpu_workspace_contract.py).

Arena: one uint8 tensor filled with 0xFF.  take(n) hands out a view of exactly n bytes at an address that is a multiple of 256 (what a
kernel's alignment dispatch sees with a torch allocation), with at least 64 KiB of untouched arena on either side; check() asserts that
every byte outside the views taken is still 0xFF and names the allocation, the side and the offset of the first one that is not.
0xFF bytes read as NaN in f64, f32, bf16 and f16 and as -1 in int32, so a partial slot that is read before it was written, or an output
element that no workgroup stored, shows in the result.  The arena hands no memory out twice between two reset() calls: a view stays
valid and stays out of every later view's guards.

GuardedBackend: a HipBackend whose workspaces and whose empty() outputs are views of an arena.  A workspace is exactly the stated
bytes, so the library's own size check runs at equality; a later request for the same (key, bytes) gets the same view, filled with
0xFF again (one fit asks for the 4 MiB "small" workspace dozens of times), any other size a view of its own.  The launches of one
chunked call share one workspace (HipBackend._chunked_launch takes it once), so it is poisoned again before each of them.  Use it
inside guarded(monkeypatch, arena), which points the module-level _scratch of backend.py and kfold.py at the arena for the workspaces
that do not go through HipBackend._workspace.  Only what empty() allocates is guarded: outputs made with zeros() are ordinary memory.

Two rules keep this safe on a shared GPU.  The workspaces "rank1", "rank1t" and "ceiling_sink", and the keys a test names in
`plain_keys`, are torch.empty allocations of the backend's own, cached per key and outside the arena whatever _scratch is patched
to: they hold the flag words and the control block of workgroups that wait on each other, and a defect there must not be turned into
a wait.  A region that kernels read as integers is zero-filled by the test before the call (Arena.on_take), guards kept.
"""
import contextlib

import torch

from cmtf_pls_amd.backend import HipBackend

POISON = 0xFF
GUARD = 64 << 10
ALIGN = 256
ARENA_BYTES = 256 << 20
UNPOISONED_KEYS = ("rank1", "rank1t", "ceiling_sink")


class Arena:
    def __init__(self, device, nbytes=ARENA_BYTES, on_take=None):
        self.device = torch.device(device)
        self.buf = torch.empty(int(nbytes) + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = -self.buf.data_ptr() % ALIGN            # offsets count from the first 256-byte boundary of the storage
        self.nbytes = int(nbytes)
        self.on_take = on_take                               # on_take(name, view) after every take: zero-fill of integer regions
        self.reset()

    def reset(self):
        self.epoch = getattr(self, "epoch", 0) + 1           # views taken before a reset are no longer anybody's
        self.buf.fill_(POISON)
        self.views = []                                      # (name, offset, nbytes)
        self._end = 0

    def take(self, n, name="view"):
        n = int(n)
        assert n > 0, (name, n)
        off = -(-(self._end + GUARD) // ALIGN) * ALIGN
        if off + n + GUARD > self.nbytes:
            raise MemoryError(f"arena of {self.nbytes} bytes exhausted by {name} ({n} bytes at {off}, {len(self.views)} views taken): "
                              "the case is too large for this test")
        self.views.append((f"{name}#{len(self.views)}", off, n))
        self._end = off + n
        view = self.buf[self.base + off:self.base + off + n]
        assert view.data_ptr() % ALIGN == 0 and view.numel() == n
        if self.on_take is not None:
            self.on_take(name, view)
        return view

    def holds(self, t):
        """Whether tensor t lies inside the arena's storage."""
        lo = self.buf.data_ptr()
        return t.device == self.buf.device and lo <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= lo + self.buf.numel()

    def retake(self, view, name="view"):
        """A view taken since the last reset, handed out again: poisoned, then on_take as for a new one."""
        view.fill_(POISON)
        if self.on_take is not None:
            self.on_take(name, view)
        return view

    def offset_of(self, view):
        return view.data_ptr() - self.buf.data_ptr() - self.base

    def repoison(self, ptr):
        """Fill the view that starts at address ptr with 0xFF again (a workspace that several launches of one call share);
        False when ptr is not the start of a view."""
        off = ptr - self.buf.data_ptr() - self.base
        for _, o, n in reversed(self.views):
            if o == off:
                self.buf[self.base + off:self.base + off + n].fill_(POISON)
                return True
        return False

    def check(self):
        bad = self.buf[self.base:self.base + self.nbytes] != POISON
        for _, off, n in self.views:
            bad[off:off + n] = False
        if not bool(bad.any()):
            return
        first = int(bad.nonzero()[0])
        before = [v for v in self.views if v[1] + v[2] <= first]
        after = [v for v in self.views if v[1] > first]
        near = []                                            # the nearer neighbour first
        if before:
            near.append((first - (before[-1][1] + before[-1][2]), f"{first - (before[-1][1] + before[-1][2])} bytes after the end of", before[-1]))
        if after:
            near.append((after[0][1] - first, f"{after[0][1] - first} bytes before the start of", after[0]))
        near.sort(key=lambda e: e[0])
        where = " / ".join(f"{side} {v[0]} (offset {v[1]}, {v[2]} bytes)" for _, side, v in near) or "an arena without a view"
        raise AssertionError(f"guard overwritten at arena offset {first}: {where}; {int(bad.sum())} bytes in all")


class GuardedBackend(HipBackend):
    """A HipBackend on arena.device whose workspaces and empty() outputs come from `arena`."""

    def __init__(self, arena, device=None):
        super().__init__(device if device is not None else arena.device)
        self._guard(arena)

    def _guard(self, arena):
        self.arena = arena
        self.plain_keys = ()          # further keys a test keeps on ordinary memory (a waiting kernel the list above does not name)
        self._plain = {}              # key -> torch.empty buffer of an unpoisoned key
        self._taken = {}              # (arena epoch, key, nbytes) -> arena view
        self.stated = []              # (key, stated bytes, in the arena) of every _workspace call

    def _workspace(self, key, nbytes):
        nbytes = int(nbytes)
        poisoned = key not in UNPOISONED_KEYS and key not in self.plain_keys
        self.stated.append((key, nbytes, poisoned))
        if not poisoned:              # never through _scratch: guarded() has pointed that at the arena
            buf = self._plain.get(key)
            if buf is None or buf.numel() < nbytes:
                buf = self._plain[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            assert not self.arena.holds(buf)
            return buf
        n, name = (nbytes if nbytes > 0 else 256), "workspace:" + key
        view = self._taken.get((self.arena.epoch, key, n))
        if view is None:
            view = self._taken[(self.arena.epoch, key, n)] = self.arena.take(n, name)
            return view
        return self.arena.retake(view, name)

    def empty(self, *shape, dtype=torch.float64):
        shape = torch.Size(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else torch.Size(shape)
        nbytes = shape.numel() * torch.empty(0, dtype=dtype).element_size()
        if nbytes == 0:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return self.arena.take(nbytes, "empty").view(dtype).view(shape)

    def _chunked_launch(self, name, call, *args, **kwargs):
        """The chunks of one call share one workspace: poison it again before every launch, so that no chunk reads what the one
        before it left there (the probe without a workspace does not count)."""
        def poisoned(first, count, ws, nbytes):
            if ws is not None:
                assert self.arena.repoison(ws), f"{name}: the chunks' workspace is no arena view (use GuardedBackend inside guarded())"
            return call(first, count, ws, nbytes)
        return super()._chunked_launch(name, poisoned, *args, **kwargs)


def arena_scratch(arena):
    """The stand-in for backend._scratch: exactly nbytes (256 for none) from the arena."""
    def _scratch(nbytes, device):
        assert torch.device(device) == arena.device
        return arena.take(int(nbytes) if int(nbytes) > 0 else 256, "scratch")
    return _scratch


@contextlib.contextmanager
def guarded(monkeypatch, arena):
    """Inside: the workspaces that backend.py and kfold.py allocate with _scratch are views of the arena as well."""
    import cmtf_pls_amd.backend as backend_mod
    import cmtf_pls_amd.kfold as kfold_mod

    with monkeypatch.context() as m:
        m.setattr(backend_mod, "_scratch", arena_scratch(arena))
        m.setattr(kfold_mod, "_scratch", arena_scratch(arena))
        yield arena


def bits(t):
    """t as integers of its element size: NaN equals NaN, -0.0 differs from 0.0."""
    if not t.dtype.is_floating_point:
        return t
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))
