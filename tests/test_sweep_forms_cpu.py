"""CPU-only: the form every X sweep takes, asked of the library (cmtfpls_sweep_form: the host function each entry launches from,
no GPU call).  Every case of tests/sweep_cases.py selects exactly the form it names, and the table together with its EXEMPT list
names every form the library can take -- so a threshold edit in csrc/sweeps.hip that moves a case onto another kernel, or a new
form that no case reaches, fails here."""
import ctypes

import pytest

import sweep_cases as SC


@pytest.fixture(scope="module")
def form():
    import os

    from cmtf_pls_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend.sweep_form


def _case_id(c):
    op, dt, I, A, B, masked, M, name = c
    return f"{op}-{dt}-{I}x{A}x{B}-{'m' if masked else 'u'}-M{M}"


@pytest.mark.parametrize("case", SC.CASES, ids=_case_id)
def test_every_case_selects_the_form_it_names(form, case):
    op, dt, I, A, B, masked, M, name = case
    assert form(op, dt, I, A, B, masked, M) == name


@pytest.mark.parametrize("dt", SC.DTYPES)
@pytest.mark.parametrize("op", SC.OPS)
def test_table_and_exemptions_name_every_form_of_the_library(form, op, dt):
    from cmtf_pls_amd.backend import HipBackend
    listed = HipBackend.sweep_form_list(op, dt)
    assert len(listed) == len(set(listed)) > 0
    tabled = {c[7] for c in SC.CASES if c[0] == op and c[1] == dt}
    exempt = set(SC.EXEMPT.get(op, {}))
    assert len(exempt) <= 4
    assert not (tabled & exempt), "an exempt form that a case selects is not exempt"
    assert tabled | exempt == set(listed), (sorted(set(listed) - tabled - exempt), sorted((tabled | exempt) - set(listed)))


@pytest.mark.parametrize("dt", SC.DTYPES)
def test_masked_and_complete_data_are_both_tabled_for_every_form(dt):
    """The contractions' names do not say whether NaNs are skipped (MODE 0 / 1 are the same form): the table holds both."""
    for op in ("mode0_contract", "mode0_contract_yq"):
        for name in {c[7] for c in SC.CASES if c[0] == op and c[1] == dt and not c[7].startswith("unsupported")}:
            assert {c[5] for c in SC.CASES if c[0] == op and c[1] == dt and c[7] == name} == {False, True}, (op, name)


def test_declines_by_name(form):
    """What the GPU tests assert by shape (the backend returns None), by name."""
    # score_deflate beyond one workgroup: P > 1024 x 16 vectors (f32 65536, f64 32768); scalar rows: 1024 x 16 elements
    assert form("score_deflate", "f32", 9, 256, 256) == "rows1024 nv16 KC FULL parked"
    assert form("score_deflate", "f32", 9, 256, 260) == "unsupported: row does not fit one workgroup"
    assert form("score_deflate", "f64", 9, 128, 256) == "rows1024 nv16 KC FULL parked"
    assert form("score_deflate", "f64", 9, 128, 258) == "unsupported: row does not fit one workgroup"
    assert form("score_deflate", "f32", 9, 128, 129) == "unsupported: row does not fit one workgroup"      # 16512 scalar elements
    assert form("score_deflate", "f32", 9, 127, 129) == "rows1024 nv16 scalar parked"                      # 16383
    # loadings + the parked half row (128 KB) + 1 KB beyond 160 KB: more than 3968 doubles of loadings
    assert form("score_deflate", "f32", 3, 4, 5000) == "unsupported: loadings + the parked half row exceed the LDS"
    assert form("score_deflate", "f32", 3, 8, 3960) == "rows1024 nv16 vec parked"                          # 8 + 3960 = 3968
    assert form("score_deflate", "f32", 3, 8, 3964) == "unsupported: loadings + the parked half row exceed the LDS"
    assert form("score_deflate", "f32", 3, 4, 3000, True) == "rows1024 nv4 vec masked"                     # nothing parked: no such limit
    assert form("score_deflate", "f32", 3, 1, 12292) == "unsupported: loadings exceed LDS"
    # the scalar shape of mode0_contract_yq and M > 64
    assert form("mode0_contract_yq", "f32", 40, 7, 9, False, 3) == "unsupported: scalar shape"
    assert form("mode0_contract_yq", "f64", 40, 7, 9, True, 3) == "unsupported: scalar shape"
    assert form("mode0_contract_yq", "f32", 40, 1, 64, False, 65) == "unsupported: more than 64 responses"
    assert form("mode0_contract_yq", "f32", 40, 1, 64, False, 64) == "narrow yq"
    assert form("mode0_contract_yq", "f32", 333, 1, 30724, False, 65) == "unsupported: more than 64 responses"   # no up-front u either
    assert form("score_gram", "f32", 20, 4, 8, False, 65) == "unsupported: more than 64 responses"
    assert form("score_gram", "f32", 20, 4, 8, False, 64) == "narrow nvl1 op0 gram"
    assert form("deflate_contract_yq", "f32", 40, 7, 9, False, 3) == "unsupported: not a 16-byte vector shape"
    assert form("deflate_contract_yq", "f32", 40, 4, 8, False, 65) == "unsupported: more than 64 responses"


def test_misaligned_x_takes_the_scalar_walks(form):
    """The row sweeps fall back to element accesses when X is not 16-byte aligned; the contractions refuse it."""
    assert form("score", "f32", 100, 4, 8, aligned16=False) == "wave scalar"
    assert form("deflate", "f32", 100, 33, 128, aligned16=False) == "wave scalar"
    assert form("center", "f64", 100, 33, 128, aligned16=False) == "wave scalar"
    assert form("score_deflate", "f32", 100, 4, 64, aligned16=False) == "rows256 nv1 scalar"
    from cmtf_pls_amd import _lib
    with pytest.raises(_lib.CmtfplsError):
        form("mode0_contract", "f32", 100, 4, 8, aligned16=False)


def test_fused_deflation_and_contraction_is_named(form):
    """deflate_contract_yq: the workgroup-per-row-segment form from 512 rows of more than 256 V 4 elements on, else the tile form."""
    assert form("deflate_contract_yq", "f32", 700, 128, 128, False, 16) == "rows1024 nv4 nseg1 KC FULL"
    assert form("deflate_contract_yq", "f32", 515, 50, 100, True, 3) == "rows1024 nv4 nseg1 vec masked"
    assert form("deflate_contract_yq", "f32", 513, 256, 256, False, 32) == "rows1024 nv4 nseg4 KC FULL"
    assert form("deflate_contract_yq", "f32", 511, 256, 256, False, 32) == "tile yqpre"
    assert form("deflate_contract_yq", "f64", 300, 16, 16, True, 16) == "tile yq masked"
    from cmtf_pls_amd.backend import HipBackend
    for dt in SC.DTYPES:
        names = HipBackend.sweep_form_list("deflate_contract_yq", dt)
        assert {"tile yq", "tile yqpre masked", "rows1024 nv4 nseg4 KC FULL", "unsupported: more than 64 responses"} <= set(names)


def test_unknown_op_and_bad_arguments_are_invalid():
    from cmtf_pls_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    EINVAL = 1
    assert lib.cmtfpls_sweep_form(b"transpose", 4, 100, 4, 8, 0, 0, 1, buf, len(buf)) == EINVAL
    assert lib.cmtfpls_sweep_form_list(b"transpose", 4, buf, len(buf)) == EINVAL
    assert lib.cmtfpls_sweep_form(None, 4, 100, 4, 8, 0, 0, 1, buf, len(buf)) == EINVAL
    assert lib.cmtfpls_sweep_form(b"score", 2, 100, 4, 8, 0, 0, 1, buf, len(buf)) == EINVAL              # no f16 storage
    assert lib.cmtfpls_sweep_form(b"score", 4, 0, 4, 8, 0, 0, 1, buf, len(buf)) == EINVAL
    assert lib.cmtfpls_sweep_form(b"score_gram", 4, 100, 4, 8, 0, 0, 1, buf, len(buf)) == EINVAL         # M = 0
    assert lib.cmtfpls_sweep_form(b"score", 4, 100, 4, 8, 0, 0, 1, buf, 4) == EINVAL                     # name does not fit
    assert lib.cmtfpls_sweep_form(b"score", 4, 100, 4, 8, 0, 0, 1, buf, len(buf)) == 0 and buf.value == b"narrow nvl1 op0"
    assert lib.cmtfpls_abi_version() == 1
