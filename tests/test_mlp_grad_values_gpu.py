"""The MlpDx gradient sweeps, what they compute: the second table of tests/golden/make_mlp_values.py - direct C-ABI calls to
dmpc_mlp2_param_grad and to dmpc_mlp_rollout_grad at both depths, over every activation, every count of hidden units per
lane, the walks past the caps on the partials, T = 2, T = 1 and absent d_x_init / d_u - against the recording
tests/golden/mlp_grad_values.npz, made from the library before the four sweeps moved into one header under one host
entry point.  Bit for bit on every output (the largest through the SHA-256 of their bytes, as the file keeps them), and the kernel
launched last per row.  A gradient row's `x` is the RECORDED `x` of its rollout row, never what the library under test rolled."""
import os

import numpy as np
import pytest

from tests.test_mlp_values_gpu import SCRIPT

pytestmark = pytest.mark.gpu

ROWS = SCRIPT.rows("grads")
with np.load(SCRIPT.NPZ_GRADS) as z:
    RECORDED = {key: z[key] for key in z.files}


@pytest.fixture(scope="module")
def taken():
    full = SCRIPT.run_rows(RECORDED, "grads")
    SCRIPT.check_conditions(full, "grads")           # on the arrays themselves, before the largest become digests
    return SCRIPT.compact(full)


def test_the_recording_covers_the_table_and_meets_its_conditions():
    """every row's kernel is its depth's reduction, nothing is non-finite, every weight gradient of a T > 1 row has a non-zero
    entry, d_u[T-1] is exactly zero and d_u[0] is not, T = 1 copies grad_x[0], a walk's last trajectory differs from its first"""
    SCRIPT.check_conditions(RECORDED, "grads")
    assert os.path.getsize(SCRIPT.NPZ_GRADS) < 256 * 1024


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_every_output_equals_the_recording(taken, row):
    for key in SCRIPT.keys(row):
        got, want = taken[key], RECORDED[key]
        if key.endswith("/kernel"):
            assert str(got) == str(want)
            continue
        assert got.dtype == want.dtype and got.shape == want.shape, key
        np.testing.assert_array_equal(got, want, err_msg=key)
        assert got.tobytes() == want.tobytes(), key      # (signed zeros and NaN payloads too)
