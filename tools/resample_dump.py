#!/usr/bin/env python3
"""Dump everything the resampling drivers return, report and ask of the backend on a fixed table of tiny models, to compare two
trees of the Python drivers bit for bit: get_q2y, kfold_predictions, get_q2y_kfold(per_component=True), permutation_test_q2y,
get_q2y_repeated_kfold, get_q2y_nested_kfold and bootstrap_factors (validate.py; kfold.py, permutation.py, repeated.py, nested.py,
bootstrap.py).  Per case and driver the dump holds every returned array, the report (q2y_report_ / bootstrap_report_) and the call
log: every HipBackend method the driver called, with the shapes and dtypes of its tensor arguments and the values of its scalar
ones, and every fit / transform / predict of a model it refitted (the backend calls inside those are not logged: a refit is one
line).  An exception is dumped as its type and text.  The package is the one next to this file, the library the one CMTFPLS_LIB
names (else the in-tree build).  Not a test: it carries no expected values (tests/test_gpu_resample_reports.py holds the reports
and call logs of this table to tests/golden/resample_reports.json).

The table (CASES) uses the smallest shapes at which the drivers' shared steps can go wrong: I = 12..36, trailing sides <= 7, M <= 3
(but for the M = 65 decline), R = 2, K = 3, float64 on host arrays:
  models     tPLS of order 2, 3 and 4 | ctPLS of a matrix + an order-3 block and of a matrix + an order-4 block | each complete and
             with a few NaNs
  switches   every EngineOptions switch that routes them, off and on: masked_folds, masked_folds_coupled, masked_tensor_folds,
             tensor_folds, tensor_folds_coupled, tensor_resamples_coupled, coupled_permutations | device_folds=False
  counts     on the device passes 23 permutations (10, 10, 3 a pass), 9 splits (ragged last pass), 24 nested models (20, 4) and
             2 min(I, 32) + 1 resamples (the last pass holds one model, run as two copies); where every model refits, 2, 1, 6 and 2
  declines   K = 33 | M = 65 | an offset of 1e6 on X (the statistics of the first build) | NaN in Y | a block of order 5 | an
             order-4 block under masked_folds / masked_folds_coupled alone
  statuses   a training row without an observed entry (a masked model that refits alone), tPLS and ctPLS
Usage: python tools/resample_dump.py OUT.json      then      python tools/resample_dump.py --compare A.json B.json
       python tools/resample_dump.py --fixture DUMP.json FIXTURE.json      (reports and call-log digests, no arrays)
--compare: every array (floats by their bits: NaN payloads and signed zeros count), report and call log of A and B by name; prints
the counts, every difference (for a float array also the largest relative one), and exits 1 on any."""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

R, K = 2, 3
SHAPES = {"t2": [(20, 7)], "t3": [(21, 5, 4)], "t4": [(22, 4, 3, 2)], "c3": [(23, 6), (23, 4, 3)], "c4": [(24, 6), (24, 3, 2, 3)],
          "t3k": [(36, 3, 2)], "t5": [(12, 3, 2, 2, 2)], "c5": [(12, 6), (12, 2, 2, 2, 2)]}
RESPONSES = {"t2": 1, "t3": 3, "t4": 2, "c3": 2, "c4": 3, "t3k": 2, "t5": 2, "c5": 2}
DRIVERS = ("get_q2y", "kfold_predictions", "get_q2y_kfold", "permutation_test_q2y", "get_q2y_repeated_kfold", "get_q2y_nested_kfold",
           "bootstrap_factors")
SMALL = {"perms": 2, "repeats": 1, "outer": 2, "resamples": 2}
COUPLED_ON = {"tensor_folds_coupled": True, "tensor_resamples_coupled": True, "coupled_permutations": True}


def _case(name, model, nan=None, options=None, small=(), device_folds=True, drivers=DRIVERS, n_splits=K, **data):
    """small: the counts that take their refit-sized value (True: all of them)."""
    return {"name": name, "model": model, "nan": nan, "options": dict(options or {}), "device_folds": device_folds,
            "small": tuple(SMALL) if small is True else tuple(small), "drivers": tuple(drivers), "n_splits": n_splits, "data": data}


CASES = [
    _case("t2/complete", "t2"),
    _case("t3/complete", "t3"),
    _case("t3/complete/device_folds_off", "t3", small=True, device_folds=False),
    _case("t4/complete/off", "t4", small=True),
    _case("t4/complete/tensor_folds", "t4", options={"tensor_folds": True}),
    _case("c3/complete/off", "c3", small=("perms",)),
    _case("c3/complete/coupled_permutations", "c3", options={"coupled_permutations": True}),
    _case("c4/complete/off", "c4", small=True),
    _case("c4/complete/tensor_folds_coupled", "c4", options={"tensor_folds_coupled": True}, small=("perms", "resamples")),
    _case("c4/complete/on", "c4", options=COUPLED_ON),
    _case("t2/nan/off", "t2", nan="few", small=True),
    _case("t2/nan/masked_folds", "t2", nan="few", options={"masked_folds": True}, small=("outer",)),
    _case("t3/nan/off", "t3", nan="few", small=True),
    _case("t3/nan/masked_folds", "t3", nan="few", options={"masked_folds": True}, small=("outer",)),
    _case("t4/nan/off", "t4", nan="few", small=True),
    _case("t4/nan/masked_folds_alone", "t4", nan="few", options={"masked_folds": True}, small=True),
    _case("t4/nan/tensor_folds_alone", "t4", nan="few", options={"tensor_folds": True}, small=True),
    _case("t4/nan/masked_tensor_folds", "t4", nan="few", options={"masked_tensor_folds": True}, small=("outer",)),
    _case("c3/nan/off", "c3", nan="few", small=True),
    _case("c3/nan/masked_folds_coupled", "c3", nan="few", options={"masked_folds_coupled": True}, small=("outer",)),
    _case("c4/nan/off", "c4", nan="few", small=True),
    _case("c4/nan/masked_folds_coupled", "c4", nan="few", options={"masked_folds_coupled": True, **COUPLED_ON}, small=True),
    _case("decline/K33", "t3k", small=True, n_splits=33, drivers=("kfold_predictions", "permutation_test_q2y", "get_q2y_repeated_kfold")),
    _case("decline/K33/coupled", "c3", small=True, n_splits=33, options={"coupled_permutations": True}, rows=36,
          drivers=("kfold_predictions", "permutation_test_q2y", "get_q2y_repeated_kfold")),
    _case("decline/M65", "t3", small=True, responses=65),
    _case("decline/offset", "t3", small=True, offset=1e6),
    _case("decline/offset/coupled", "c3", small=True, offset=1e6, options={"coupled_permutations": True}),
    _case("decline/nan_in_y", "t3", small=True, y_nan=True),
    _case("decline/nan_in_y/masked_folds", "t3", nan="few", small=True, y_nan=True, options={"masked_folds": True}),
    _case("decline/order5", "t5", small=True, options={"tensor_folds": True}),
    _case("decline/order5/coupled", "c5", small=True, options=COUPLED_ON),
    _case("status/masked_folds", "t3", nan="row", options={"masked_folds": True}, small=True),
    _case("status/masked_folds_coupled", "c3", nan="row", options={"masked_folds_coupled": True}, small=True),
]


def inputs(case, seed):
    """(the blocks the model is fitted on, Y, the blocks and Y the drivers then read): the latter differ from the former where a
    fit on them would be NaN everywhere (a row without an observed entry, NaN in Y)."""
    rng = np.random.default_rng(seed)
    shapes = SHAPES[case["model"]]
    data = case["data"]
    if "rows" in data:
        shapes = [(data["rows"],) + s[1:] for s in shapes]
    I = shapes[0][0]
    M = data.get("responses", RESPONSES[case["model"]])
    T = rng.standard_normal((I, R + 1))
    Xs = [(T @ rng.standard_normal((R + 1, int(np.prod(s[1:])))) + 0.3 * rng.standard_normal((I, int(np.prod(s[1:]))))).reshape(s)
          + data.get("offset", 0.0) for s in shapes]
    Y = T @ rng.standard_normal((R + 1, M)) + 0.3 * rng.standard_normal((I, M))
    if case["nan"] is not None:                                              # a few NaNs in every block; no row loses all entries
        for X in Xs:
            flat = X.reshape(I, -1)
            for i, j in zip(rng.choice(I, 6, replace=False), rng.integers(1, flat.shape[1], 6)):
                flat[i, j] = np.nan
    Xr, Yr = [X.copy() for X in Xs], Y.copy()
    if case["nan"] == "row":                                                 # row 4 of the last block: nothing observed
        Xr[-1][4] = np.nan
    if data.get("y_nan"):
        Yr[3, 0] = np.nan
    return Xs, Y, Xr, Yr


def model_of(case, seed, backend=None, device="cuda:0"):
    """The fitted model of a case, its training data replaced by what the drivers are to read."""
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.engine import EngineOptions
    Xs, Y, Xr, Yr = inputs(case, seed)
    coupled = case["model"].startswith("c")
    m = (ctPLS if coupled else tPLS)(R, dtype="float64", device=device, backend=backend,
                                     options=EngineOptions(small_fit=False, **case["options"]))
    m.fit(Xs if coupled else Xs[0], Y)
    if coupled:
        m.original_Xs = Xr
    else:
        m.original_X = Xr[0]
    m.original_Y = Yr
    return m


def counts_of(case, I):
    big = {"perms": 23, "repeats": 9, "outer": 6, "resamples": 2 * min(I, 32) + 1}
    return {k: (SMALL[k] if k in case["small"] else v) for k, v in big.items()}


def calls_of(case, m):
    """name -> (the driver's call, the name of the report it sets)."""
    from cmtf_pls_amd import validate as V
    n = counts_of(case, m.original_Y.shape[0])
    df, ns = case["device_folds"], case["n_splits"]
    calls = {
        "get_q2y": (lambda: V.get_q2y(m, device_folds=df), "q2y_report_"),
        "kfold_predictions": (lambda: V.kfold_predictions(m, n_splits=ns, device_folds=df), "q2y_report_"),
        "get_q2y_kfold": (lambda: V.get_q2y_kfold(m, n_splits=ns, per_component=True, device_folds=df), "q2y_report_"),
        "permutation_test_q2y": (lambda: V.permutation_test_q2y(m, n_permutations=n["perms"], n_splits=ns, per_component=True,
                                                                device_folds=df), "q2y_report_"),
        "get_q2y_repeated_kfold": (lambda: V.get_q2y_repeated_kfold(m, n_splits=ns, n_repeats=n["repeats"], per_component=True,
                                                                    device_folds=df), "q2y_report_"),
        "get_q2y_nested_kfold": (lambda: V.get_q2y_nested_kfold(m, n_outer=n["outer"], n_inner=3 if n["outer"] > 2 else 2,
                                                                device_folds=df), "q2y_report_"),
        "bootstrap_factors": (lambda: V.bootstrap_factors(m, n_resamples=n["resamples"], device_folds=df), "bootstrap_report_"),
    }
    return {k: calls[k] for k in case["drivers"]}


# ---- the recorder -------------------------------------------------------------------------------------------------------------------
def describe(a):
    import torch
    if isinstance(a, torch.Tensor):
        return f"{str(a.dtype).replace('torch.', '')}{list(a.shape)}"
    if isinstance(a, np.ndarray):
        return f"np.{a.dtype}{list(a.shape)}"
    if isinstance(a, ctypes.Array):
        return "[" + ", ".join(describe(v) for v in a) + "]"
    if isinstance(a, ctypes.Structure):
        ints = [f"{f}={getattr(a, f)}" for f, t in a._fields_ if t is ctypes.c_int]
        return f"{type(a).__name__}({', '.join(ints)})"
    if isinstance(a, (list, tuple)):
        return "[" + ", ".join(describe(v) for v in a) + "]"
    if isinstance(a, dict):
        return "{" + ", ".join(f"{k}: {describe(v)}" for k, v in a.items()) + "}"
    if isinstance(a, (np.integer, np.floating, np.bool_)):
        return repr(a.item())
    if a is None or isinstance(a, (bool, int, float, str)):
        return repr(a)
    return type(a).__name__


@contextlib.contextmanager
def recording(classes, log):
    """Every public method of `classes` (name -> (class, the methods to wrap; None: all)) logs its outermost call into `log`."""
    depth = [0]
    saved = []

    def wrap(label, fn):
        def wrapped(self, *args, **kwargs):
            if depth[0] == 0:
                parts = [describe(v) for v in args] + [f"{k}={describe(v)}" for k, v in kwargs.items()]
                log.append(f"{label}({', '.join(parts)})")
            depth[0] += 1
            try:
                return fn(self, *args, **kwargs)
            finally:
                depth[0] -= 1
        return wrapped

    for cname, (cls, names) in classes.items():
        for name in (names if names is not None else [n for n, v in vars(cls).items() if callable(v) and not n.startswith("_")]):
            fn = vars(cls)[name]
            saved.append((cls, name, fn))
            setattr(cls, name, wrap(f"{cname}.{name}", fn))
    try:
        yield
    finally:
        for cls, name, fn in saved:
            setattr(cls, name, fn)


def flatten(prefix, v, out):
    if isinstance(v, dict):
        for k, x in v.items():
            flatten(f"{prefix}/{k}" if prefix else str(k), x, out)
    elif isinstance(v, (list, tuple)) and any(isinstance(x, (np.ndarray, list, tuple, dict)) for x in v):
        for j, x in enumerate(v):
            flatten(f"{prefix}/{j}", x, out)
    else:
        a = np.ascontiguousarray(np.asarray(v))
        out[prefix] = {"dtype": str(a.dtype), "shape": list(a.shape), "hex": a.tobytes().hex()}


def plain(v):
    """A report as JSON holds it."""
    def default(o):
        if isinstance(o, (np.integer, np.floating, np.bool_)):
            return o.item()
        if isinstance(o, np.ndarray):
            return o.tolist()
        raise TypeError(type(o).__name__)
    return json.loads(json.dumps(v, default=default))


def run_case(case, seed, classes, backend=None, device="cuda:0"):
    """driver -> {"arrays", "report", "calls"} (or "raises") of one case."""
    m = model_of(case, seed, backend, device)
    out = {}
    for name, (call, report) in calls_of(case, m).items():
        log, arrays = [], {}
        for attr in ("q2y_report_", "bootstrap_report_"):
            if hasattr(m, attr):
                delattr(m, attr)
        with recording(classes, log):
            try:
                flatten("", {"result": call()}, arrays)
                got = {"arrays": arrays, "report": plain(getattr(m, report, None))}
            except Exception as e:                                             # its type and text are part of the behaviour
                got = {"raises": f"{type(e).__name__}: {e}"}
        out[name] = dict(got, calls=log)
    return out


def hip_classes():
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.backend import HipBackend
    models = ["fit", "transform", "predict"]
    return {"HipBackend": (HipBackend, None), "tPLS": (tPLS, models), "ctPLS": (ctPLS, models)}


def digest(calls):
    """What the fixture keeps of a call log: its length, the SHA-256 of its lines and the number of calls per method."""
    per = {}
    for line in calls:
        per[line.split("(", 1)[0]] = per.get(line.split("(", 1)[0], 0) + 1
    return {"n": len(calls), "sha256": hashlib.sha256("\n".join(calls).encode()).hexdigest(), "methods": dict(sorted(per.items()))}


def fixture_of(dump):
    return {case: {drv: {k: (digest(v) if k == "calls" else v) for k, v in got.items() if k != "arrays"} for drv, got in drivers.items()}
            for case, drivers in dump.items()}


def main(out_path):
    import time
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cmtf_pls_amd import _lib
    classes = hip_classes()
    dump, t0 = {}, time.perf_counter()
    for seed, case in enumerate(CASES, start=1):
        t1 = time.perf_counter()
        dump[case["name"]] = run_case(case, seed, classes)
        forms = {d: (g["raises"] if "raises" in g else (g["report"] or {}).get("form", "")[:60]) for d, g in dump[case["name"]].items()}
        print(f"{case['name']}: {time.perf_counter() - t1:.2f} s", flush=True)
        for d, f in forms.items():
            print(f"    {d}: {f}", flush=True)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(dump, f)
    n = sum(len(g.get("arrays", {})) for c in dump.values() for g in c.values())
    print(f"{n} arrays, {sum(len(c) for c in dump.values())} driver runs of {len(dump)} cases in {time.perf_counter() - t0:.1f} s -> "
          f"{out_path}; library {_lib.LIB_PATH}")


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad, n_arrays, n_runs = [], 0, 0
    for case in sorted(set(a) | set(b)):
        for drv in sorted(set(a.get(case, {})) | set(b.get(case, {}))):
            x, y = a.get(case, {}).get(drv), b.get(case, {}).get(drv)
            n_runs += 1
            if x is None or y is None:
                bad.append(f"{case}/{drv}: only in {'A' if y is None else 'B'}")
                continue
            for key in ("raises", "report"):
                if x.get(key) != y.get(key):
                    bad.append(f"{case}/{drv}: {key}: {x.get(key)!r} != {y.get(key)!r}")
            if x["calls"] != y["calls"]:
                first = next((i for i, (p, q) in enumerate(zip(x["calls"], y["calls"])) if p != q), min(len(x["calls"]), len(y["calls"])))
                bad.append(f"{case}/{drv}: call logs ({len(x['calls'])} and {len(y['calls'])} lines) part at line {first}: "
                           f"{x['calls'][first:first + 1]} != {y['calls'][first:first + 1]}")
            xa, ya = x.get("arrays", {}), y.get("arrays", {})
            for k in sorted(set(xa) | set(ya)):
                n_arrays += 1
                if xa.get(k) == ya.get(k):
                    continue
                note = ""
                if k in xa and k in ya and xa[k]["dtype"] == ya[k]["dtype"] == "float64" and xa[k]["shape"] == ya[k]["shape"]:
                    p, q = (np.frombuffer(bytes.fromhex(v[k]["hex"]), dtype=np.float64) for v in (xa, ya))
                    with np.errstate(all="ignore"):
                        note = f" (largest relative difference {np.nanmax(np.abs(p - q) / np.maximum(np.abs(p), 1e-300)):.3g})"
                bad.append(f"{case}/{drv}: array {k}{note}")
    print(f"{n_arrays} arrays, {n_runs} reports and call logs of {len(set(a) | set(b))} cases compared: "
          f"{'all identical' if not bad else str(len(bad)) + ' differ'}")
    for line in bad:
        print("  differs:", line)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 4 and sys.argv[1] == "--fixture":
        with open(sys.argv[3], "w") as f:
            json.dump(fixture_of(json.load(open(sys.argv[2]))), f, indent=0, sort_keys=True)
        sys.exit(0)
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main(sys.argv[1])
