"""The line-search kernels, what they compute: the table of tests/golden/make_search_values.py - one direct C-ABI call per
search kernel, every batch with a trajectory accepted at once, some accepted after several passes and one that is still
worse at the cap - against the recording tests/golden/search_values.npz, made from the library before those kernels were
last changed.  Bit for bit on every output, and the kernel launched last per row, so a row cannot stop covering its kernel
unnoticed.  Rows under a latched DMPC_NO_* switch run in a fresh child process per switch."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu


def load_script():
    spec = importlib.util.spec_from_file_location("make_search_values", os.path.join(GOLDEN, "make_search_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SCRIPT = load_script()
ROWS = SCRIPT.rows()
with np.load(SCRIPT.NPZ) as z:
    RECORDED = {key: z[key] for key in z.files}
SCALES = {r["id"]: RECORDED[r["id"] + "/ks_scale"].tolist() for r in ROWS}


@pytest.fixture(scope="module")
def taken(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("search_values")
    got = SCRIPT.run_rows(None, SCALES)
    scales_path = str(tmp / "scales.json")
    with open(scales_path, "w") as fh:
        json.dump(SCALES, fh)
    for switch in SCRIPT.SWITCHES:       # one process at a time
        got.update(SCRIPT.run_child(switch, scales_path, str(tmp / (switch + ".npz"))))
    return got


def test_the_recording_covers_the_table_and_the_epilogue():
    assert sorted(RECORDED) == sorted("%s/%s" % (r["id"], k) for r in ROWS for k in SCRIPT.OUTPUTS + ("kernel", "ks_scale"))
    for r in ROWS:
        n_ls, info = RECORDED[r["id"] + "/n_ls"], RECORDED[r["id"] + "/info"]
        assert r["kernel"] in str(RECORDED[r["id"] + "/kernel"]), r["id"]
        assert n_ls[-1] == SCRIPT.CAP and info[-1] & 8, (r["id"], "the last trajectory hits the cap")     # DMPC_INFO_LS_ITERCAP
        assert not (info[:-1] & 8).any() and len(set(n_ls[:-1].tolist())) >= 2, (r["id"], n_ls, "two pass counts below the cap")
        assert n_ls[0] == 1, (r["id"], "the first trajectory is accepted at once")


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_every_output_equals_the_recording(taken, row):
    got = taken[row["id"]]
    assert got["kernel"] == str(RECORDED[row["id"] + "/kernel"])
    for k in SCRIPT.OUTPUTS:
        want = RECORDED["%s/%s" % (row["id"], k)]
        assert got[k].dtype == want.dtype, k
        np.testing.assert_array_equal(got[k], want, err_msg=k)
        assert got[k].tobytes() == want.tobytes(), k      # (signed zeros and NaN payloads too)
