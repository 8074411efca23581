"""tests/arena.py without a GPU: fake "calls" - plain Python on CPU tensors - that break the memory contract one way each must
be reported, a clean one must not; and every entry point of the C ABI that takes a device pointer has a row in the case table
of the memory-contract test (tests/abi_calls.py)."""
import ctypes

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import _lib
from tests import abi_calls
from tests.arena import BAND, FILL_B, GUARD, Builder


def declare(b):
    return dict(x=b.inp("x", np.arange(6.0)), m=b.inp("m", [1, 0, 1], np.uint8), y=b.out("y", (5,)), z=b.out("z", (2, 3), np.float64),
                n=b.out("n", (3,), np.int32), keep=b.inout("keep", [1.0, 2.0, 3.0], unwritten=[False, True, False]),
                ws=b.ws("ws", 40), info=b.info("info", 2))


def clean(a, h):
    """y = 2 x[:5], z = 1, n = 0..2, keep's ends bumped, the workspace scribbled over, a flag or-ed in"""
    a.view(h["ws"]).fill_(7)
    a.view(h["y"]).copy_(2 * a.view(h["x"])[:5])
    a.view(h["z"]).fill_(1.0)
    a.view(h["n"]).copy_(torch.arange(3, dtype=torch.int32))
    a.view(h["keep"])[0] += 1
    a.view(h["keep"])[2] += 1
    a.view(h["info"])[1] |= 2
    return 0


def raw(a, h, offset, nbytes):
    """bytes of the arena relative to the start of an array (negative: before it)"""
    o = a.offset[h.name] + offset
    return a.buf[o:o + nbytes]


def past_the_end(a, h):
    clean(a, h)
    raw(a, h["y"], h["y"].nbytes, 4).view(torch.float32).fill_(3.0)           # one float written just past an output
    return 0


def before_the_start(a, h):
    clean(a, h)
    raw(a, h["z"], -16, 16).fill_(0)                                         # 16 bytes written before an output
    return 0


def element_left_out(a, h):
    rc = clean(a, h)
    a.view(h["y"]).view(torch.int32)[3] = GUARD if a.layout == "A" else FILL_B   # one output element left unwritten
    return rc


def reads_stale_workspace(a, h):
    stale = int(a.view(h["ws"])[:4].clone().view(torch.int32)[0])            # a workspace word the call never wrote
    clean(a, h)
    a.view(h["y"])[0] = float(stale % 1000)
    return 0


def input_modified(a, h):
    clean(a, h)
    a.view(h["m"])[1] = 9
    return 0


def unwritten_region_touched(a, h):
    clean(a, h)
    a.view(h["keep"])[1] = 0.0
    return 0


def refused_but_wrote(a, h):
    a.view(h["n"])[2] = 5
    return -2


def refused(a, h):
    return -1


def run(fake, layout):
    b = Builder()
    h = declare(b)
    a = b.build(layout, "cpu")
    a.snapshot()
    rc = fake(a, h)
    return a, a.check(rc)


def findings(fake):
    (a, fa), (b, fb) = run(fake, "A"), run(fake, "B")
    return fa, fb, a.compare(b)


def test_layouts_alignment_and_views():
    for layout in "AB":
        b = Builder()
        h = declare(b)
        a = b.build(layout, "cpu")
        base = a.buf.data_ptr()
        order = list(h.values()) if layout == "A" else list(h.values())[::-1]
        offs = [a.offset[s.name] for s in order]
        assert offs == sorted(offs) and offs[0] == (256 if layout == "A" else 16)
        for s, nxt in zip(order, order[1:]):
            gap = a.offset[nxt.name] - (a.offset[s.name] + s.nbytes)
            assert BAND[layout] <= gap < BAND[layout] + 16
        assert a.nbytes - (offs[-1] + order[-1].nbytes) >= BAND[layout]
        for s in h.values():
            v = a.view(s)
            assert v.data_ptr() == a.ptr(s) == base + a.offset[s.name] and a.ptr(s) % 16 == 0
            assert tuple(v.shape) == s.shape and v.element_size() == s.dtype.itemsize
        assert a.ptr(None) is None
        words = a.buf.view(torch.int32).numpy()
        assert (words[a.guard_mask.reshape(-1, 4).all(axis=1)] == GUARD).all()
        fill = GUARD if layout == "A" else FILL_B
        assert (a.view(h["y"]).view(torch.int32) == fill).all() and (a.view(h["z"]).view(torch.int32) == fill).all()
        assert (a.view(h["info"]) == 0).all() and a.view(h["x"]).tolist() == list(range(6))
    # the guard word is a quiet NaN with a payload as float32; doubled it is NOT a NaN as float64 (the exponent field is 0x7FC,
    # not 0x7FF) but 3.04e307, within a factor of 60 of the largest double: poison all the same.  Layout B's fill is 12345678.0f
    assert np.isnan(np.array([GUARD], np.int32).view(np.float32)[0])
    assert 3.0e307 < np.array([GUARD, GUARD], np.int32).view(np.float64)[0] < 3.1e307
    assert np.array([FILL_B], np.int32).view(np.float32)[0] == np.float32(12345678.0)


def test_a_clean_call_reports_nothing():
    assert findings(clean) == ([], [], [])
    assert findings(refused) == ([], [], [])


@pytest.mark.parametrize("fake,array,word", [(past_the_end, "y", "guard"), (before_the_start, "z", "guard"),
                                             (input_modified, "m", "input modified at byte 1"),
                                             (unwritten_region_touched, "keep", "declared unwritten changed at byte 7"),
                                             (refused_but_wrote, "n", "refused call (rc -2) wrote byte 8")])
def test_violations_seen_in_either_layout(fake, array, word):
    fa, fb, _ = findings(fake)
    for f in (fa, fb):
        assert len(f) == 1 and array in f[0] and word in f[0], f
    if fake is past_the_end:
        assert "1 bytes past the end of y" in fa[0]
    if fake is before_the_start:
        assert "16 bytes before z" in fa[0], fa


def test_an_element_left_unwritten_is_seen_in_layout_a():
    fa, fb, fc = findings(element_left_out)
    assert fa == ["y: not written at byte 12 (1 words left)"] and fb == []
    assert len(fc) == 1 and fc[0].startswith("y: layouts differ at element 3 (byte 12)")


def test_an_output_that_depends_on_stale_workspace_differs_between_the_layouts():
    assert GUARD % 1000 != FILL_B % 1000
    fa, fb, fc = findings(reads_stale_workspace)
    assert fa == [] and fb == []
    assert len(fc) == 1 and fc[0].startswith("y: layouts differ at element 0 (byte 0)")


def test_a_sum_within_its_tolerance_is_not_a_difference():
    def make(v):
        b = Builder()
        s = b.out("s", (2,), tol=1e-4)
        a = b.build("A", "cpu")
        a.snapshot()
        a.view(s).copy_(torch.tensor(v))
        assert a.check(0) == []
        return a
    assert make([1.0, 200.0]).compare(make([1.00005, 200.01])) == []
    assert len(make([1.0, 200.0]).compare(make([1.0002, 200.0]))) == 1
    assert len(make([1.0, float("nan")]).compare(make([1.0, 200.0]))) == 1


def test_every_entry_point_with_a_device_pointer_has_a_memory_contract_case():
    """a new entry point cannot be added to the binding without a row in tests/abi_calls.py"""
    with_pointers = {name for name, (_, args) in _lib.SIGNATURES.items() if ctypes.c_void_p in args}
    assert "dmpc_last_kernel_name" not in with_pointers and len(with_pointers) >= 30
    covered = {c.entry for c in abi_calls.CASES}
    assert with_pointers - covered == set(), "no memory-contract case for %s" % sorted(with_pointers - covered)
    assert covered - with_pointers == set()
    assert [c.id for c in abi_calls.CASES if "lqr" in c.meta] == ["lqr:" + c["id"] for c in abi_calls.ROUTES.cases()]


def test_every_row_of_the_table_declares_its_arrays_and_matches_its_signature():
    """no GPU: each row's `make` runs (its data, its workspace queries), every call has as many arguments as the binding's
    signature, every array is cut 16-byte aligned in both layouts and no arena reaches 8 MiB"""
    from tests.arena import Spec
    lib = _lib.load()
    for c in abi_calls.CASES:
        b = Builder()
        prepare, call = c.make(b, lib)
        calls = [cl for cl in (prepare or []) + [call] if not callable(cl)]
        assert callable(call) or call[0] == c.entry, c.id
        for entry, args in calls:
            assert len(args) == len(_lib.SIGNATURES[entry][1]), (c.id, entry)
            handles = [a for a in args if isinstance(a, Spec)]
            assert all(h in b.specs for h in handles), c.id
        for layout in "AB":
            a = b.build(layout, "cpu")
            assert all(a.ptr(s) % 16 == 0 for s in b.specs), c.id
            assert a.nbytes < 8 << 20, (c.id, a.nbytes)


def test_float32_autograd_is_within_float32_of_float64_on_the_param_step_inputs():
    """the yardstick of tests/test_abi_memory_gpu.py::test_il_param_step_against_float64_autograd, a CPU computation: torch's
    float32 route (autograd + RMSprop) against its float64 route on the same inputs, max |delta| / max(1, |ref|) over grad,
    params and ms.  Measured: 1.6e-8 (kind 1, n_sc 1) to 1.07e-6 (kind 3, n_sc 4: two products with the observation matrix,
    entries up to 4, on the way there and back) over the eight (kind, n_sc) pairs; asserted: the float32 route does differ
    (the kernel's allowance, 4 times this, is no zero), and by no more than 64 roundings, 64 * 2^-24 = 3.8e-6."""
    for kind, n in abi_calls.IL_KINDS:
        d = abi_calls.il_step_data(kind, n)
        dist = abi_calls.distance(abi_calls.param_step_reference(kind, n, d, torch.float32),
                                  abi_calls.param_step_reference(kind, n, d, torch.float64))
        print("param_step kind %d n_sc %d: float32 autograd against float64 %.3e" % (kind, n, dist))
        assert 0 < dist <= 64 * 2.0 ** -24
