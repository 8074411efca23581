"""The MlpDx kernels, what they compute: the table of tests/golden/make_mlp_values.py - direct C-ABI calls to the rollout with
its linearisation, the search, the box-DDP chain with the network inside it and the weight gradient, over both depths, every
activation and every count of hidden units per lane - against the recording tests/golden/mlp_values.npz, made from the
library before those kernels were last changed.  Bit for bit on every output, and the kernel launched last per row.  A search
row's `states` and a gradient row's `x` are the RECORDED `x` of its rollout row, never what the library under test rolled."""
import importlib.util
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu


def load_script():
    spec = importlib.util.spec_from_file_location("make_mlp_values", os.path.join(GOLDEN, "make_mlp_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SCRIPT = load_script()
ROWS = SCRIPT.rows()
with np.load(SCRIPT.NPZ) as z:
    RECORDED = {key: z[key] for key in z.files}


@pytest.fixture(scope="module")
def taken():
    return SCRIPT.run_rows(RECORDED)


def test_the_recording_covers_the_table_and_meets_its_conditions():
    """every row's kernel is the instance the row is there for, every F has an entry off [I|0], every search row has a
    trajectory accepted at once and one accepted after several passes below the cap, nothing is non-finite"""
    SCRIPT.check_conditions(RECORDED)
    assert os.path.getsize(SCRIPT.NPZ) < 256 * 1024


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_every_output_equals_the_recording(taken, row):
    for key in SCRIPT.keys(row):
        got, want = taken[key], RECORDED[key]
        if key.endswith("/kernel"):
            assert str(got) == str(want)
            continue
        assert got.dtype == want.dtype, key
        np.testing.assert_array_equal(got, want, err_msg=key)
        assert got.tobytes() == want.tobytes(), key      # (signed zeros and NaN payloads too)
