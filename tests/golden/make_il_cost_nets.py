#!/usr/bin/env python
"""Generate tests/golden/il_cost_nets.npz by running the UNMODIFIED reference's env_dx/pendulum_net.py on the numpy
`chainer` stand-in (oracle/refshim), in the build container:

    python tests/golden/make_il_cost_nets.py

For each of the four cost nets and each parameter set (zeros; standard normal draws of RandomState(11 + case)), the
(Q, p) that the net's `forward` hands to `IL_Env.mpc` / `IL_Env.mpc_Q` is captured by an environment stand-in whose
`mpc` / `mpc_Q` record their arguments (the logit net passes the diagonal q, stored as diag(q)).  Stored: the parameter
values and (Q, p) in float64, keyed `<kind>_<case>_{learn_q_logit,learn_p,lower_without_diag,Q,p}`.  Data only.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.refshim import load_reference  # noqa: E402

NAMES = ("Pendulum_Net_cost_logit", "Pendulum_Net_cost_lower_triangle", "Pendulum_Net_cost_logit_strange_obervation",
         "Pendulum_Net_cost_lower_triangle_strange_obervation")
PARAMS = ("learn_q_logit", "learn_p", "lower_without_diag")
N_SC, T, B, NU = 4, 3, 2, 1


def arr(v):
    return np.asarray(getattr(v, "array", v), dtype=np.float64)


class RecordingEnv:
    """what pendulum_net.py's forward calls: env.true_dx and env.mpc(dx, x, q, p, u_init) / env.mpc_Q(dx, x, Q, p, u_init)"""
    true_dx = None

    def mpc(self, dx, xinit, q, p, u_init=None):
        self.Q, self.p = np.diag(arr(q)), arr(p)
        return None, None

    def mpc_Q(self, dx, xinit, Q, p, u_init=None):
        self.Q, self.p = arr(Q), arr(p)
        return None, None


def main():
    load_reference.load()
    import importlib
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pn = importlib.import_module("pendulum_net")
    out = {"n_sc": N_SC}
    for kind, name in enumerate(NAMES):
        for case in range(2):
            net = getattr(pn, name)(N_SC)
            rng = np.random.RandomState(11 + case)
            for prm in PARAMS:
                if hasattr(net, prm):
                    v = getattr(net, prm)
                    if case:
                        v.array[...] = rng.randn(*v.array.shape)
                    out["%d_%d_%s" % (kind, case, prm)] = arr(v).copy()
            env = RecordingEnv()
            net.forward(np.zeros((B, 3)), env, np.zeros((B, T, NU)))
            out["%d_%d_Q" % (kind, case)] = env.Q
            out["%d_%d_p" % (kind, case)] = env.p
    path = os.path.join(HERE, "il_cost_nets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
