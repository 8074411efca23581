"""CPU: what the two stream generators emit (csrc/gen_lqr_asm.py -> lqr_asm_gen.hpp, csrc/gen_mpc_fwd_asm.py ->
mpc_fwd_asm_gen.hpp) is the text whose hashes tests/golden/asm_streams.json holds - under the default knobs and under
every knob set the experiment scripts use.  The generated text decides the device code of every kernel that includes it, so
a change to the generators that is meant to move no instruction is proved here, without a compiler.  Recorded by
scripts/record_asm_streams.py, whose functions this file uses; nothing is written outside tmp_path."""
import functools
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chainer_differentiable_mpc_amd", "csrc")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load(os.path.join(ROOT, "scripts", "record_asm_streams.py"), "record_asm_streams")
GOLDEN = json.load(open(rec.GOLDEN))
CASES = [(header, env) for header, sets in rec.KNOB_SETS.items() for env in sets]


@functools.lru_cache(maxsize=None)
def default_text(header):
    return rec.generate(header, {})


def test_the_golden_holds_exactly_the_knob_sets():
    for header, sets in rec.KNOB_SETS.items():
        assert sorted(GOLDEN[header]["knob_sets"]) == sorted(rec.knob_key(env) for env in sets)


@pytest.mark.parametrize("header,env", CASES, ids=["%s:%s" % (h.split("_asm")[0], rec.knob_key(e)) for h, e in CASES])
def test_generated_header_is_the_pinned_one(header, env):
    text = default_text(header) if not env else rec.generate(header, env)
    got, want = rec.hashes(text, per_struct=not env), GOLDEN[header]
    if not env:
        moved = sorted(k for k in set(got["structs"]) | set(want["structs"]) if got["structs"].get(k) != want["structs"].get(k))
        assert not moved, "specialisations of %s whose text differs from the pinned one: %s" % (header, moved)
    assert got["sha256"] == want["knob_sets"][rec.knob_key(env)], "%s differs outside its specialisations" % header


def test_forms_for_yields_exactly_the_specialisations_of_the_header():
    if CSRC not in sys.path:
        sys.path.insert(0, CSRC)
    import gen_lqr_asm as gen
    knobs = gen.Knobs.from_env({})
    names = [form.struct_name(nx, nu) for nx, nu in gen.SHAPES for form in gen.forms_for(nx, nu, knobs)]
    assert len(names) == len(set(names))
    assert names == list(rec.structs(default_text("lqr_asm_gen.hpp")))          # the same ones, in the header's order
    assert sorted(names) == sorted(GOLDEN["lqr_asm_gen.hpp"]["structs"])


@pytest.mark.parametrize("script,header,env", [
    ("gen_lqr_asm.py", "lqr_asm_gen.hpp", {"GEN_RING_DEPTH": "4", "GEN_TIMING": "1"}),
    ("gen_mpc_fwd_asm.py", "mpc_fwd_asm_gen.hpp", {"GEN_FWD_ROW_MASK": "0"}),
])
def test_the_environment_reaches_the_knobs_of_the_script(script, header, env, tmp_path):
    out = tmp_path / header
    e = {k: v for k, v in os.environ.items() if not k.startswith("GEN_")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(CSRC, script), "--out", str(out)], env=e, check=True, capture_output=True)
    assert hashlib.sha256(out.read_bytes()).hexdigest() == GOLDEN[header]["knob_sets"][rec.knob_key(env)]
