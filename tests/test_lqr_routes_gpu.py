"""The LQR solve dispatch, what runs: the case table of tests/golden/make_lqr_routes.py through the C ABI - return code and
the kernel launched last (`dmpc_last_kernel_name`; None: nothing was launched) - against the recording
tests/golden/lqr_routes.json, made before the dispatch was last changed."""
import json

import pytest

from tests.test_lqr_routes_cpu import load_script

pytestmark = pytest.mark.gpu

SCRIPT = load_script()
with open(SCRIPT.JSON) as fh:
    RECORDED = json.load(fh)


@pytest.fixture(scope="module")
def taken():
    return {row["id"]: row for row in SCRIPT.run_cases()}


def test_the_recording_covers_the_case_table():
    assert [row["id"] for row in RECORDED] == [c["id"] for c in SCRIPT.cases()]
    assert all(row["kernel"] is None for row in RECORDED if row["rc"] < 0), "a refused call launches nothing"


@pytest.mark.parametrize("row", RECORDED, ids=[row["id"] for row in RECORDED])
def test_return_code_and_kernel_equal_the_recording(taken, row):
    assert taken[row["id"]] == row
