"""The LQR solve dispatch, what a caller is told: `dmpc_lqr_kernel_family`, `dmpc_lqr_solve_path`,
`dmpc_lqr_saving_available` and `dmpc_lqr_workspace_bytes` over a grid of 110,760 sizes, with no switch set and with each
DMPC_NO_* switch of the solve family set alone (a child process each: the switches are latched), against the recording
tests/golden/told_lqr_routes.npz (tests/golden/make_lqr_routes.py, made before the dispatch was last changed).  No GPU needed."""
import numpy as np

from tests.helpers import load_routes_script

# dmpc_lqr_solve_path over the grid with no switch set, as the recording was made
PATH_HISTOGRAM = {-2: 9960, 0: 50640, 1: 488, 2: 40, 3: 328, 4: 256, 5: 120, 6: 208, 7: 26321, 8: 19440, 9: 2959}


load_script = load_routes_script


def test_told_paths_equal_the_recording(tmp_path):
    script = load_script()
    recorded = script.load_recorded()
    paths, counts = np.unique(recorded["none"]["path"], return_counts=True)
    assert dict(zip(paths.tolist(), counts.tolist())) == PATH_HISTOGRAM
    got = script.query_children(str(tmp_path))
    for label in script.LABELS:
        for field in script.FIELDS:
            np.testing.assert_array_equal(got[label][field], recorded[label][field], err_msg="%s, %s" % (label, field))
