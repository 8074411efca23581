"""CPU: what `dmpc_box_ddp`'s dyn_kind 2 (the MlpDx network inside the box-DDP chain) decides before its first launch, the
packed weight buffer of `MlpDx.packed_weights`, and the `device_loop` argument.  No GPU is needed: every refused call returns
before the first HIP call, on pointers that are never dereferenced."""
import copy
import ctypes
import pickle

import pytest
import torch

from chainer_differentiable_mpc_amd import MlpDx, _lib
from tests import box_ddp_mlp_cases as cases
from tests.helpers import tie_rows

P = 4096          # a dummy device pointer: 16-byte aligned, never dereferenced by a refused call


def call(lib, T=4, B=2, nx=3, nu=1, F=P, f=None, dyn_kind=2, params=(5.0, 0.0, 1.0, 0.0), coupled=0, short=0):
    need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
    dp = None if params is None else ctypes.cast((ctypes.c_float * len(params))(*params), ctypes.c_void_p)
    return lib.dmpc_box_ddp(T, B, nx, nu, P, P, P, F, f, dyn_kind, dp, P, P, P, 1e-3, 5, 0.2, 10, 1e-4, 2, 20, 1, coupled,
                            P, P, P, P, P, P, P, need - short, None, None)


def test_dyn_kind_2_argument_errors_are_reported_before_any_launch():
    lib = _lib.load()
    assert call(lib, F=None) == _lib.E_BADARG
    assert call(lib, f=P) == _lib.E_BADARG
    assert call(lib, params=None) == _lib.E_BADARG
    assert call(lib, params=(5.5, 0.0, 1.0, 0.0)) == _lib.E_BADARG
    assert call(lib, params=(-1.0, 0.0, 1.0, 0.0)) == _lib.E_BADARG
    assert call(lib, params=(5.0, 0.5, 1.0, 0.0)) == _lib.E_BADARG
    assert call(lib, params=(5.0, 0.0, 2.0, 0.0)) == _lib.E_BADARG
    assert call(lib, params=(5.0, 0.0, 1.0, 0.5)) == _lib.E_BADARG
    assert call(lib, params=(float("nan"), 0.0, 1.0, 0.0)) == _lib.E_BADARG
    assert call(lib, F=P + 4) == _lib.E_BADARG                              # not 16-byte aligned
    assert call(lib, params=(300.0, 0.0, 1.0, 0.0)) == _lib.E_UNSUPPORTED
    assert call(lib, params=(0.0, 0.0, 1.0, 0.0)) == _lib.E_UNSUPPORTED
    assert call(lib, params=(5.0, 1.0, 1.0, 0.0)) == _lib.E_UNSUPPORTED     # act 1 is never assigned
    assert call(lib, params=(5.0, 5.0, 1.0, 0.0)) == _lib.E_UNSUPPORTED
    assert call(lib, nx=17) == _lib.E_UNSUPPORTED
    assert call(lib, nu=9) == _lib.E_UNSUPPORTED
    assert call(lib, coupled=1) == _lib.E_UNSUPPORTED
    assert call(lib, dyn_kind=3) == _lib.E_UNSUPPORTED
    assert call(lib, dyn_kind=-1) == _lib.E_UNSUPPORTED
    for sl in (0.0, 1.0):                                                   # every argument in order but the workspace
        assert call(lib, params=(5.0, 0.0, 1.0, sl), short=1) == _lib.E_WORKSPACE
        assert call(lib, params=(256.0, 4.0, 0.0, sl), nx=16, nu=8, short=1) == _lib.E_WORKSPACE


def test_the_workspace_query_does_not_depend_on_the_dynamics():
    lib = _lib.load()
    assert lib.dmpc_box_ddp_workspace_bytes(7, 5, 3, 1) > 0
    assert lib.dmpc_version() == 411


def model(**kw):
    return MlpDx(3, 2, 7, seed=3, **kw)


def test_packed_weights_are_the_four_tensors_in_the_order_of_the_abi():
    m = model()
    with torch.no_grad():
        m.b1.copy_(torch.arange(7.0))
        m.b2.copy_(torch.arange(3.0) - 9.0)
    flat = m.packed_weights("cpu")
    assert flat.dtype == torch.float32 and flat.dim() == 1 and flat.is_contiguous() and not flat.requires_grad
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in (m.W1, m.b1, m.W2, m.b2)]))
    assert flat.numel() == 7 * 5 + 7 + 3 * 7 + 3
    assert m.host_params()[:3] == (7.0, 0.0, 1.0) and m.host_params()[3] in (0.0, 1.0) and len(m.host_params()) == 4
    assert MlpDx(3, 2, 7, residual=False, activation="silu").host_params()[:3] == (7.0, 3.0, 0.0)


def test_packed_weights_keep_their_address_and_follow_an_in_place_step():
    m = model()
    first = m.packed_weights("cpu")
    address, before = first.data_ptr(), first.clone()
    assert m.packed_weights("cpu").data_ptr() == address
    with torch.no_grad():
        m.W1.mul_(0.9)
    again = m.packed_weights("cpu")
    assert again.data_ptr() == address
    assert torch.equal(again[:35], m.W1.detach().reshape(-1)) and not torch.equal(again[:35], before[:35])
    assert torch.equal(again[35:], before[35:])
    assert torch.equal(first, again)                                        # the same memory: refilled in place


def test_packed_weights_are_no_state_of_the_module():
    m = model()
    m.packed_weights("cpu")
    assert sorted(m.state_dict()) == ["W1", "W2", "b1", "b2"]
    assert len(list(m.parameters())) == 4 and len(list(m.buffers())) == 0


@pytest.mark.parametrize("clone", [copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m))], ids=["deepcopy", "pickle"])
def test_a_copied_model_packs_into_a_buffer_of_its_own(clone):
    m = model(device_loop=True)
    mine = m.packed_weights("cpu")
    other = clone(m)
    assert other.device_loop is True and other._packed == {}
    theirs = other.packed_weights("cpu")
    assert theirs.data_ptr() != mine.data_ptr() and torch.equal(theirs, mine)
    with torch.no_grad():
        other.W2.add_(1.0)
    assert not torch.equal(other.packed_weights("cpu"), m.packed_weights("cpu"))
    assert m.packed_weights("cpu").data_ptr() == mine.data_ptr()
    x, u = torch.randn(4, 3), torch.randn(4, 2)
    with torch.no_grad():
        assert torch.equal(clone(m)(x, u), m(x, u))


def test_device_loop_defaults_to_false_and_from_sequential_passes_it_on():
    assert MlpDx(3, 1, 5).device_loop is False and MlpDx(3, 1, 5, device_loop=True).device_loop is True
    assert "device_loop" not in repr(MlpDx(3, 1, 5)) and "device_loop=True" in repr(MlpDx(3, 1, 5, device_loop=True))
    assert "activation=tanh" in repr(MlpDx(3, 1, 5, device_loop=True))
    net = torch.nn.Sequential(torch.nn.Linear(4, 6), torch.nn.ReLU(), torch.nn.Linear(6, 3))
    assert MlpDx.from_sequential(net, 3, 1).device_loop is False
    m = MlpDx.from_sequential(net, 3, 1, device_loop=True)
    assert m.device_loop is True and m.activation == "relu"
    assert torch.equal(m.packed_weights("cpu")[:24], net[0].weight.detach().reshape(-1))


@pytest.mark.parametrize("key", cases.ONE_ITERATION, ids=cases.name)
def test_the_one_iteration_cases_have_no_tie_row(key):
    """what tests/test_box_ddp_mlp_gpu.py's one-iteration parity test relies on, decided by the float64 oracle: no row's
    accepting margin is a tie, and the relu case linearises away from every kink"""
    ref = cases.oracle_one_iteration(key)
    assert tie_rows(ref["old_costs"], ref["costs"]).sum() == 0
    if key[0] == "relu":
        assert ref["min_abs_z"] >= cases.KINK_MARGIN
