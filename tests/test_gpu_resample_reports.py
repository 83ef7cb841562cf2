"""The resampling drivers against their recorded behaviour: every row of tools/resample_dump.py's table (tiny tPLS and ctPLS models
of order 2 to 5, complete and with NaNs, every EngineOptions switch that routes them off and on, ragged and one-model last passes,
a decline from each kind of source, masked models that refit alone) through get_q2y, kfold_predictions, get_q2y_kfold,
permutation_test_q2y, get_q2y_repeated_kfold, get_q2y_nested_kfold and bootstrap_factors.  tests/golden/resample_reports.json holds,
per row and driver, the report (q2y_report_ / bootstrap_report_: form, counts, x_reads, n_iter, why) or the exception's type and
text, and of the call log -- every HipBackend method the driver called with the shapes and dtypes of its tensor arguments and the
values of its scalar ones, every fit / transform of a model it refitted -- the length, the SHA-256 of its lines and the calls per
method.  The fixture was written by `tools/resample_dump.py --fixture` from the drivers as they stood before they shared their
route, pass builder and report; equality is asserted, so a driver that takes another route, words a report differently,
or makes another sequence of backend calls fails here.  The arrays the drivers return are compared bit for bit by the tool's
--compare, not here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("resample_dump", os.path.join(ROOT, "tools", "resample_dump.py"))
DUMP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DUMP)


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "resample_reports.json")) as f:
        return json.load(f)


def test_the_fixture_holds_the_table(recorded):
    assert set(recorded) == {c["name"] for c in DUMP.CASES}
    for case in DUMP.CASES:
        assert set(recorded[case["name"]]) == set(case["drivers"])


@pytest.mark.parametrize("seed,case", list(enumerate(DUMP.CASES, start=1)), ids=[c["name"] for c in DUMP.CASES])
def test_reports_and_backend_calls_are_the_recorded_ones(seed, case, recorded):
    got = DUMP.run_case(case, seed, DUMP.hip_classes())
    want = recorded[case["name"]]
    for driver, run in got.items():
        kept = DUMP.fixture_of({"case": {driver: run}})["case"][driver]
        assert kept.get("raises") == want[driver].get("raises"), driver
        assert kept.get("report") == want[driver].get("report"), driver
        assert kept["calls"] == want[driver]["calls"], (driver, run["calls"])
