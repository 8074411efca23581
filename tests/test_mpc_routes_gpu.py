"""The MPC step dispatch, what runs: the case table of tests/golden/make_mpc_routes.py through the C ABI - return code and
the kernel launched last (`dmpc_last_kernel_name`; None: nothing was launched) - against the recording
tests/golden/mpc_routes.json, made before the dispatch was last changed.  The latched DMPC_NO_* switches each get the same
table in a fresh child process of their own; the recording keeps a switch's rows that differ from the run with none set."""
import importlib.util
import json
import os

import pytest

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu


def load_script():
    spec = importlib.util.spec_from_file_location("make_mpc_routes", os.path.join(GOLDEN, "make_mpc_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SCRIPT = load_script()
with open(SCRIPT.JSON) as fh:
    RECORDED = json.load(fh)
BASE = RECORDED["none"]


@pytest.fixture(scope="module")
def taken():
    return {row["id"]: row for row in SCRIPT.run_cases()}


def test_the_recording_covers_the_case_table():
    ids = [c["id"] for c in SCRIPT.cases()]
    assert [row["id"] for row in BASE] == ids
    assert sorted(RECORDED) == sorted(["none"] + SCRIPT.SWITCHES)
    for label in SCRIPT.SWITCHES:
        assert set(row["id"] for row in RECORDED[label]) <= set(ids), label
    assert all(row["kernel"] is None for rows in RECORDED.values() for row in rows if row["rc"] < 0), "a refused call launches nothing"


@pytest.mark.parametrize("row", BASE, ids=[row["id"] for row in BASE])
def test_return_code_and_kernel_equal_the_recording(taken, row):
    assert taken[row["id"]] == row


@pytest.mark.parametrize("switch", SCRIPT.SWITCHES)
def test_the_table_under_a_switch_equals_the_recording(switch, tmp_path):
    rows = SCRIPT.run_child(switch, str(tmp_path / "rows.json"))
    assert [row["id"] for row in rows] == [row["id"] for row in BASE]
    assert SCRIPT.changed(rows, BASE) == RECORDED[switch]
