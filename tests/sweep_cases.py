"""One table of shapes for the X sweeps of csrc/sweeps.hip, shared by tests/test_sweep_forms_cpu.py (every case selects the form it
names; the table covers every form the library lists) and tests/test_gpu_sweep_forms.py (every case against float64).

A case is (op, dtype, I, A, B, masked, M, form): X is (I, A B) of dtype "f32" | "f64", `form` is the name cmtfpls_sweep_form gives
for it.  For the contractions only P = A B matters (A = 1); for "center", masked means "rowcnt is wanted"; M is the number of
responses of the entries that take Y (0 elsewhere).  A form "unsupported: ..." is a decline: the entry returns
CMTFPLS_EUNSUPPORTED and the backend method None.

Constants of the derivations: 256 threads per workgroup of the contraction, V = 4 (f32) | 2 (f64) elements per 16-byte vector, a
column tile of 256 V U elements (U = 2 | 4 column groups per thread), 1024 workgroups aimed at by the guarded contraction, 512 by
the guard-free (FULL) one and 256 when there are >= 16 tiles of 4 groups and I tiles <= 2^21; U = 4 when a workgroup then still
gets >= 128 rows; rows interleave (ilv) and u = Y q is formed up front (yqpre) from 16 column tiles on.  The row sweeps run 512
workgroups: one round is 2048 rows for the wavefront-per-row kernels, 512 for the workgroup-per-row kernels, 512 / nseg for the
segmented centring and 16384 / nvl for the short-row kernel; I = 2 rounds + 37 gives three rounds with a ragged last one (the
red[parity] buffers of score_deflate_kernel and center_rows_kernel are reused in the third), I = round + 37 where a row is longer
than 100 KB and nothing is carried between rounds.

Where a threshold depends on V the f64 twin halves B, so both storage types sit at the same point of the dispatch."""

OPS = ("colstats", "mode0_contract", "mode0_contract_yq", "center", "score", "score_gram", "deflate", "score_deflate")
DTYPES = ("f32", "f64")

CASES = []


def _add(op, dt, I, A, B, masked, M, form):
    CASES.append((op, dt, I, A, B, bool(masked), M, form))


def _twin(dt, b32, b64):
    return b32 if dt == "f32" else b64


# ---- contractions ---------------------------------------------------------------------------------------------------------------
# (I, P for f32, P for f64, form) -- every one with many row blocks and a ragged last one unless it says otherwise
_CONTRACT = [
    (40000, 48, 48, "narrow"),                                  # 1000 row blocks of 40 rows; 21 / 10 rows per workgroup pass
    (5000, 1301, 1301, "scalar"),                               # 6 column tiles x 167 row blocks of 30 rows
    (5000, 2052, 1026, "vec U2 guarded blocks1024"),            # 2 tiles, the second 4 / 2 columns wide; 313 blocks of 16, the last of 8
    (5000, 2048, 1024, "vec U2 FULL blocks512"),                # one exact tile of 2 groups, not of 4; 313 blocks of 16
    (130060, 516, 258, "vec U4 guarded blocks1024"),            # ceil(130060 / 1024) = 128 rows: the first U4 shape; 270 MB
    (65040, 4096, 2048, "vec U4 FULL blocks512"),               # ceil(65040 / 512) = 128; 1.07 GB
    (2051, 65536, 32768, "vec U4 FULL ilv blocks256"),          # 16 tiles x 16 row blocks of ceil(2051 / 16) = 129 rows; 540 MB
    (333, 30724, 15362, "vec U2 guarded ilv blocks1024"),       # 16 tiles of 2 groups (8 of 4: 16-row blocks), the last 4 / 2 columns
    (333, 32768, 16384, "vec U2 FULL ilv blocks512"),           # 16 exact tiles of 2 groups; 32 row blocks
    (8140, 61444, 30722, "vec U4 guarded ilv blocks1024"),      # 16 tiles of 4 groups, ceil(8140 / 64) = 128 rows; 2.0 GB
]
_STATS = ("narrow", "scalar", "vec U2 guarded blocks1024", "vec U2 FULL blocks512")     # the statistics pass stays at U = 2, never ilv

for _dt in DTYPES:
    for _I, _p32, _p64, _form in _CONTRACT:
        _P = _twin(_dt, _p32, _p64)
        if _form in _STATS:
            _add("colstats", _dt, _I, 1, _P, True, 0, _form)
        for _m in (False, True):
            _add("mode0_contract", _dt, _I, 1, _P, _m, 0, _form)
            if _form == "scalar":
                continue
            _yq = _form + (" yqpre" if " ilv" in _form else " yq")
            for _M in ((5, 64) if _I == 333 and _p32 == 30724 else (5,)):
                _add("mode0_contract_yq", _dt, _I, 1, _P, _m, _M, _yq)
    for _m in (False, True):
        # more than 2048 rows per workgroup: ceil(2097189 / 1024) = 2049, the second LDS chunk of u holds one row
        _add("mode0_contract_yq", _dt, 2097189, 1, 8, _m, 5, "narrow yq chunks")
    _add("mode0_contract_yq", _dt, 40, 7, 9, False, 3, "unsupported: scalar shape")
    _add("mode0_contract_yq", _dt, 40, 1, 64, False, 65, "unsupported: more than 64 responses")

# ---- score, score_gram, deflate: wavefront per row (one round = 2048 rows), short rows, loadings from global memory --------------
_NARROW = [(8229, 8, 128, 64, 4), (16421, 4, 128, 64, 2), (32805, 2, 128, 64, 1)]       # (I, A, B f32, B f64, nvl): 2 rounds + 37
_WAVE = [(4133, 4, 260, "wave vec"), (4133, 4, 261, "wave scalar"),
         (2085, 3, 12292, "wave vec GL"), (2085, 3, 12293, "wave scalar GL")]             # A + B > 12288 doubles: beyond 96 KB of LDS

for _dt in DTYPES:
    for _m in (False, True):
        _sfx = " masked" if _m else ""
        for _I, _A, _B, _form in _WAVE:
            _add("score", _dt, _I, _A, _B, _m, 0, _form + _sfx)
            for _M in ((64,) if "GL" in _form else (1, 64)):
                _add("score_gram", _dt, _I, _A, _B, _m, _M, _form + " gram" + _sfx)
        for _I, _A, _b32, _b64, _nvl in _NARROW:
            _add("score", _dt, _I, _A, _twin(_dt, _b32, _b64), _m, 0, f"narrow nvl{_nvl} op0" + _sfx)
            _add("score_gram", _dt, _I, _A, _twin(_dt, _b32, _b64), _m, 5, f"narrow nvl{_nvl} op0 gram" + _sfx)
            _add("score_deflate", _dt, _I, _A, _twin(_dt, _b32, _b64), _m, 0, f"narrow nvl{_nvl} op2" + _sfx)
    _add("score_gram", _dt, 20, 4, 8, False, 65, "unsupported: more than 64 responses")
    for _I, _A, _B, _form in _WAVE:
        _add("deflate", _dt, _I, _A, _B, False, 0, _form)
    for _I, _A, _b32, _b64, _nvl in _NARROW:
        _add("deflate", _dt, _I, _A, _twin(_dt, _b32, _b64), False, 0, f"narrow nvl{_nvl} op1")
    # deflate_rows_kernel: rows of (256 V 4, 1024 V 4] and (1024 V 4, 1024 V 16] elements; KC: 1024 V % B == 0
    for _A, _b32, _b64, _form in [(33, 128, 64, "rows1024 nv4 KC"), (50, 100, 50, "rows1024 nv4 vec"),
                                  (130, 128, 64, "rows1024 nv16 KC"), (170, 100, 50, "rows1024 nv16 vec")]:
        _add("deflate", _dt, 1061, _A, _twin(_dt, _b32, _b64), False, 0, _form)

# ---- score_deflate: one workgroup per row (one round = 512 rows) -------------------------------------------------------------------
# (A, B f32, B f64, form); scalar shapes (odd B) have V = 1 for both storage types
_SD = [
    (5, 51, 51, "rows256 nv1 scalar"),                          # 255 <= 256 elements
    (7, 99, 99, "rows256 nv4 scalar"),                          # 693 in (256, 1024]
    (13, 100, 50, "rows256 nv4 vec"),                           # 1300 in (1024, 4096], 1024 % 100 != 0
    (3, 512, 256, "rows256 nv4 KC"),                            # 1536: the stride is a multiple of B, the row is not covered exactly
    (64, 64, 32, "rows256 nv4 KC FULL"),                        # 4096 = 256 x 4 x 4
    (3, 1001, 1001, "rows1024 nv4 scalar"),                     # 3003 in (1024, 4096]
    (50, 100, 50, "rows1024 nv4 vec"),                          # 5000 in (4096, 16384]
    (33, 128, 64, "rows1024 nv4 KC"),
    (128, 128, 64, "rows1024 nv4 KC FULL"),                     # 16384 = 1024 x 4 x 4
    (200, 75, 75, "rows1024 nv16 scalar parked"),               # 15000 in (4096, 16384]
    (101, 99, 99, "rows1024 nv16 scalar parked"),               # 9999: a walk that wraps B in every step
    (150, 200, 100, "rows1024 nv16 vec parked"),                # 30000 in (16384, 65536]
    (100, 256, 128, "rows1024 nv16 KC parked"),                 # ragged: 25600 of 65536
    (256, 256, 128, "rows1024 nv16 KC FULL parked"),            # 65536 = 1024 x 4 x 16; 278 MB
]
for _dt in DTYPES:
    for _m in (False, True):
        for _A, _b32, _b64, _form in _SD:
            _add("score_deflate", _dt, 1061, _A, _twin(_dt, _b32, _b64), _m, 0, _form + (" masked" if _m else ""))
    _add("score_deflate", _dt, 3, 1, 12292, False, 0, "unsupported: loadings exceed LDS")                 # 12294 doubles > 96 KB
    _add("score_deflate", _dt, 3, 300, 300, False, 0, "unsupported: row does not fit one workgroup")       # 90000 > 1024 x 4 x 16
    _add("score_deflate", _dt, 3, 4, 5000, False, 0, "unsupported: loadings + the parked half row exceed the LDS")   # 40 KB + 128 KB

# ---- center ------------------------------------------------------------------------------------------------------------------------
# (I, A, B f32, B f64, form).  center_kernel: rows of <= 256 V 4 elements (vec: P % V == 0) -- and any row that no nseg <= 64 with
# 512 % nseg == 0 and P % (nseg V) == 0 cuts into segments of <= 1024 V 4, such as (1, 70000): 5, 6, 7 do not divide 512 and
# 70000 = 2^4 x 4375 is no multiple of 8 V.  center_rows_kernel: one round = 512 / nseg rows.
_CENTER = [
    (4133, 4, 260, 260, "wave vec"),
    (4133, 3, 261, 261, "wave scalar"),                         # P = 783 (4 x 261 = 1044 is a vector shape: P counts, not B)
    (300, 1, 70000, 70000, "wave vec"),
    (1061, 33, 128, 64, "rows1024 nv4 nseg1"),
    (549, 128, 256, 128, "rows1024 nv4 nseg2"),
    (293, 256, 256, 128, "rows1024 nv4 nseg4"),
    (165, 1, 72000, 36000, "rows1024 nv4 nseg8"),               # ragged: segments of 9000 = 2 x 4096 + 808 (f64: 4500 = 2 x 2048 + 404)
    (101, 1, 200000, 100000, "rows1024 nv4 nseg16"),            # 13 segments would do; 16 is the next divisor of 512
    (69, 1, 400000, 200000, "rows1024 nv4 nseg32"),
    (53, 1, 800000, 400000, "rows1024 nv4 nseg64"),
]
for _dt in DTYPES:
    for _I, _A, _b32, _b64, _form in _CENTER:
        for _m in (False, True):
            _add("center", _dt, _I, _A, _twin(_dt, _b32, _b64), _m, 0, _form + (" rowcnt" if _m else ""))

# Forms the library lists that no case selects: {op: {form: the smallest selecting shape and why it is left out}}.  At most 4 per op.
EXEMPT = {
    "mode0_contract": {
        "vec U4 FULL ilv blocks512": "I = 131073, P = 65536 f32 (>= 16 exact tiles of 4 groups and I tiles > 2^21): 34 GB",
    },
    "mode0_contract_yq": {
        "vec U4 FULL ilv blocks512 yqpre": "I = 131073, P = 65536 f32, as for mode0_contract: 34 GB",
        "vec U4 guarded blocks1024 yq chunks": "I = 2097153, P = 516 f32 (more than 2048 rows per workgroup at one column tile): 4.3 GB",
        "vec U4 FULL blocks512 yq chunks": "I = 1048577, P = 4096 f32 (more than 2048 rows at 512 workgroups): 17 GB; run by "
                                           "test_gpu_kernels.py::test_mode0_contract_yq_row_chunks at 270000 x 16384",
    },
}
