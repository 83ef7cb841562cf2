"""The harness of tests/guarded_memory.py has teeth: an Arena on the CPU notices one byte on either side of a view and names the view
and the side; and the failure the poison is there for -- a reduce that reads a partial slot no tile stored -- is written down as a
ten-line torch stand-in that is right on a zero-filled workspace and wrong on a poisoned one."""
import pytest
import torch

from guarded_memory import ALIGN, GUARD, POISON, UNPOISONED_KEYS, Arena, GuardedBackend, arena_scratch, bits, guarded, same_bits

CPU = torch.device("cpu")
SMALL = 1 << 20


def test_clean_use_passes():
    a = Arena(CPU, SMALL)
    a.check()
    v = a.take(1000, "ws")
    w = a.take(24, "out").view(torch.float64)
    v.zero_()
    w.fill_(1.5)
    a.check()
    a.reset()
    assert not a.views and bool((a.buf == POISON).all())
    a.check()


@pytest.mark.parametrize("n", [1, 3, 24, 255, 256, 257, 4096 + 8])
def test_view_is_exact_and_aligned(n):
    a = Arena(CPU, SMALL)
    prev_end = 0
    for k in range(3):
        v = a.take(n, f"v{k}")
        off = a.offset_of(v)
        assert v.numel() == n and v.dtype == torch.uint8
        assert off % ALIGN == 0 and v.data_ptr() % ALIGN == 0
        assert off - prev_end >= GUARD and a.nbytes - (off + n) >= GUARD        # untouched arena before and after
        assert bool((v == POISON).all())
        prev_end = off + n


def test_arena_does_not_grow():
    a = Arena(CPU, SMALL)
    with pytest.raises(MemoryError, match="too large for this test"):
        a.take(SMALL - GUARD, "big")
    a.take(SMALL - 2 * GUARD - ALIGN, "fits")
    a.check()


@pytest.mark.parametrize("side", ["after", "before"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_byte_outside_a_view_fails_and_is_named(side, which):
    a = Arena(CPU, SMALL)
    views = [a.take(n, f"alloc{k}") for k, n in enumerate((40, 1000, 8))]
    for v in views:
        v.zero_()
    a.check()
    off = a.offset_of(views[which])
    at = off + views[which].numel() if side == "after" else off - 1
    a.buf[a.base + at] = 0
    want = (f"1 bytes before the start of alloc{which}#{which} " if side == "before" else f"0 bytes after the end of alloc{which}#{which} ")
    with pytest.raises(AssertionError) as e:
        a.check()
    msg = str(e.value)
    assert f"arena offset {at}:" in msg and msg.split(": ", 1)[1].startswith(want) and "1 bytes in all" in msg, msg
    a.buf[a.base + at] = POISON
    a.check()


def test_far_guard_bytes_are_checked_too():
    a = Arena(CPU, SMALL)
    a.take(64, "only")
    a.buf[a.base + a.nbytes - 1] = 7                          # the last byte of the arena
    with pytest.raises(AssertionError, match="after the end of only#0"):
        a.check()
    a.buf[a.base + a.nbytes - 1] = POISON
    a.buf[a.base] = 7                                         # the first
    with pytest.raises(AssertionError, match="arena offset 0: 65536 bytes before the start of only#0"):
        a.check()


def test_on_take_and_repoison():
    seen = []
    a = Arena(CPU, SMALL, on_take=lambda name, view: (seen.append((name, view.numel())), view[-8:].zero_()))
    v = a.take(64, "ws")
    assert seen == [("ws", 64)] and bool((v[:-8] == POISON).all()) and bool((v[-8:] == 0).all())
    w = a.take(16, "out")
    assert a.repoison(v.data_ptr()) and bool((v == POISON).all())
    assert not a.repoison(v.data_ptr() + 8)                   # not the start of a view
    w.zero_()
    a.check()


def test_scratch_stand_in_takes_the_stated_bytes():
    a = Arena(CPU, SMALL)
    scratch = arena_scratch(a)
    assert scratch(1000, CPU).numel() == 1000 and scratch(0, CPU).numel() == 256
    a.check()


def _bare_backend(arena):
    """GuardedBackend's allocation side without a GPU or the library: HipBackend.__init__ needs both, _workspace and empty neither."""
    be = GuardedBackend.__new__(GuardedBackend)
    be.device = arena.device
    be._guard(arena)
    return be


def test_waiting_kernels_workspaces_stay_outside_the_arena(monkeypatch):
    """Inside guarded() -- where backend._scratch itself hands out arena views -- the keys of kernels whose workgroups wait on each
    other, and a test's plain_keys, are ordinary cached memory without poison; every other key is an exact, poisoned arena view."""
    import cmtf_pls_amd.backend as backend_mod
    a = Arena(CPU, SMALL)
    be = _bare_backend(a)
    be.plain_keys = ("score_contract",)
    with guarded(monkeypatch, a):
        assert a.holds(backend_mod._scratch(100, CPU))                          # what HipBackend._workspace would have been given
        for key in UNPOISONED_KEYS + be.plain_keys:
            ws = be._workspace(key, 1000)
            assert not a.holds(ws) and ws.numel() >= 1000, key
            ws.zero_()
            assert be._workspace(key, 900).data_ptr() == ws.data_ptr(), key      # cached per key, as HipBackend's
            assert not a.holds(be._workspace(key, 5000)), key                    # and grown outside the arena too
        inside = be._workspace("contract", 1000)
        assert a.holds(inside) and inside.numel() == 1000 and bool((inside == POISON).all())
        a.check()
    assert [(k, p) for k, _, p in be.stated if k in ("rank1", "score_contract", "contract")] == \
        [("rank1", False)] * 3 + [("score_contract", False)] * 3 + [("contract", True)]


def test_a_workspace_asked_for_again_is_the_same_view_poisoned_again():
    a = Arena(CPU, SMALL)
    be = _bare_backend(a)
    first = be._workspace("small", 4096)
    first.zero_()
    again = be._workspace("small", 4096)
    assert again.data_ptr() == first.data_ptr() and again.numel() == 4096 and bool((again == POISON).all())
    other = be._workspace("small", 4095)                                         # another size: the stated bytes exactly, a view of its own
    assert other.data_ptr() != first.data_ptr() and other.numel() == 4095
    assert be._workspace("press_rows", 0).numel() == 256
    assert len(a.views) == 3
    a.reset()
    fresh = be._workspace("small", 4096)                                         # after a reset nothing is remembered
    assert len(a.views) == 1 and a.offset_of(fresh) == a.views[0][1]
    a.check()


def test_empty_is_an_exact_poisoned_view():
    a = Arena(CPU, SMALL)
    be = _bare_backend(a)
    t = be.empty(3, 5, dtype=torch.float32)
    assert a.holds(t) and t.shape == (3, 5) and a.views[-1][2] == 60 and bool(torch.isnan(t).all())
    assert be.empty((2, 2)).dtype == torch.float64 and be.empty(0).numel() == 0
    a.check()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
def test_poison_reads_as_nan(dtype):
    a = Arena(CPU, SMALL)
    assert bool(torch.isnan(a.take(64, "f").view(dtype)).all())
    assert bool((a.take(64, "i").view(torch.int32) == -1).all())


def test_bits_compare_nan_and_signed_zero():
    nan = torch.tensor([float("nan"), 1.0], dtype=torch.float64)
    assert not torch.equal(nan, nan.clone()) and same_bits(nan, nan.clone())
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert bits(torch.arange(3, dtype=torch.int32)).dtype == torch.int32


# ---- the failure mode: "partials then reduce" with the store of an empty tile skipped ------------------------------------------------
def _partials_then_reduce(x, tile, ws, store_empty_tiles):
    """sum(x) as a kernel pair would form it: tile k stores the sum of its rows into ws[k], the reduce adds all ntiles slots.  The
    grid is sized for 4 more rows than x has (a caller that rounds up), so the last tile can be empty."""
    ntiles = -(-(x.numel() + 4) // tile)
    part = ws.view(torch.float64)[:ntiles]
    for k in range(ntiles):
        rows = x[k * tile:(k + 1) * tile]
        if rows.numel() or store_empty_tiles:
            part[k] = rows.sum()
    return part.sum()


def test_skipped_store_of_an_empty_tile_shows_only_on_poison():
    x = torch.arange(1.0, 25.0, dtype=torch.float64)         # 24 rows in tiles of 8: the grid of 4 tiles has an empty last one
    want = x.sum()
    zeroed = torch.zeros(4 * 8, dtype=torch.uint8)
    assert _partials_then_reduce(x, 8, zeroed, store_empty_tiles=False) == want           # a fresh mapping hides the defect
    a = Arena(CPU, SMALL)
    got = _partials_then_reduce(x, 8, a.take(4 * 8, "partials"), store_empty_tiles=False)
    assert got != want and bool(torch.isnan(got))                                          # the poison does not
    assert _partials_then_reduce(x, 8, a.take(4 * 8, "partials"), store_empty_tiles=True) == want
    a.check()
