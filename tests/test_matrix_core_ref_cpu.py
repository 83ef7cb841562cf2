"""The dispatch mirrors of tests/matrix_core_ref.py against the case tables that tests/test_gpu_matrix_core_limits.py runs on
the device: every case selects the instance it names, turns its grid over where it claims to, and has the chunk count its
comment states.  No GPU."""
import matrix_core_ref as MC


def _instance(st, I, A, B, R):
    return MC.mttkrp_mixed_instance(I, A, B, R) if st == "mixed" else MC.mttkrp_instance(st, I, A, B, R)


def test_every_mttkrp_case_selects_the_instance_it_names():
    for st, (A, B), R, inst, Is in MC.SAMPLE_CASES:
        for I in Is:
            assert _instance(st, I, A, B, R) == inst, (st, A, B, R, I)
            assert MC.mttkrp_rounds(inst, I) == -(-I // 8192) >= 2
        # X is at most 1.2 GB (f32 272 x 128 at 8193 samples); every other case stays under 540 MB
        assert max(Is) * A * B * (8 if st == "f64" else 4) <= 1.2e9
    st, (A, B), R, inst, (I,) = MC.NOT_PER_SAMPLE
    assert _instance(st, I, A, B, R) == inst and MC.mttkrp_rounds(inst, I) == 1
    for st, (A, B), R, by_i in MC.TILE_CASES:
        for I, inst in by_i.items():
            assert _instance(st, I, A, B, R) == inst and MC.mttkrp_rounds(inst, I) == 2, (st, A, B, R, I)


def test_per_sample_instances_are_all_reached_or_known_unreachable():
    """Every (form, parameters) that run_mttkrp can select for some shape, found by enumeration, is in the case table."""
    seen = set()
    for st in ("f32", "f64"):
        for A in range(16, 257, 16):
            for B in range(8, 513, 8):
                for R in range(1, 17):
                    inst = MC.mttkrp_instance(st, 8193, A, B, R)
                    if inst is not None and inst[0] != "tile":
                        seen.add((st,) + inst)
    covered = {(st,) + inst for st, _, _, inst, _ in MC.SAMPLE_CASES if st != "mixed"}
    assert seen == covered
    assert not any(i[1] == "jk" and i[2] == 8 for i in seen) and not any(i[1] == "kj4" and i[3] == 4 for i in seen)


def test_chunk_counts_of_the_per_sample_cases():
    """Odd counts end in the tail branch of the b0 / b1 loop, even ones in the pair loop's `more ? xs : xs_next`; 3 and 17 take
    both."""
    n = {(st, ab, R): MC.sample_chunks(inst, "f32" if st == "mixed" else st, *ab) for st, ab, R, inst, _ in MC.SAMPLE_CASES}
    assert n[("f32", (32, 256), 16)] == 4 and n[("f64", (16, 128), 10)] == 2
    assert n[("f32", (16, 128), 14)] == 1 and n[("f32", (32, 64), 14)] == 1 and n[("f64", (16, 64), 10)] == 1
    assert n[("f32", (16, 192), 10)] == 3 and n[("f64", (16, 96), 10)] == 3 and n[("f32", (16, 64), 10)] == 1
    assert n[("mixed", (48, 128), 10)] == 3 and n[("mixed", (32, 64), 7)] == 1 and n[("mixed", (272, 128), 5)] == 17


def test_mixed_mttkrp_edges():
    assert MC.mttkrp_mixed_instance(40, 16, 16, 33) is None
    assert MC.mttkrp_mixed_instance(40, 1, 769, 16) is None and MC.mttkrp_mixed_instance(40, 1, 768, 16) is None
    assert MC.mttkrp_mixed_instance(40, 1, 767, 16) == ("tile_mixed", False, 1)
    assert MC.mttkrp_mixed_instance(40, 256, 384, 16) == ("kj_mixed", 2)
    assert MC.mttkrp_mixed_instance(40, 272, 384, 16) == ("tile_mixed", True, 1)
    assert MC.mttkrp_mixed_instance(40, 16, 128, 10, base=4) == ("tile_mixed", False, 1)


def test_xcov_cases_select_the_plan_and_instances_they_name():
    for name, (I, P, M), plan, insts in MC.XCOV_CASES + [MC.XCOV_BIG]:
        assert MC.plan_xcov(I, P) == plan, name
        for st, mixed, off in (("f32", True, 4), ("f32", False, 4), ("f64", False, 16)):
            base = off if "misaligned" in name else 0
            assert [t[2] for t in MC.xcov_instances(st, I, P, M, base=base, mixed=mixed)] == insts, (name, st, mixed)
        assert MC.xcov_workspace_bytes(I, P, M) == plan[2] * min(M, 64) * P * 8
    assert MC.plan_xcov(4096, 16384) == (64, 256, 16) and MC.plan_xcov(1030, 128 * 128) == (64, 128, 9)
