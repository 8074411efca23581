#!/usr/bin/env python
"""Pin what the two stream generators emit: tests/golden/asm_streams.json holds, for lqr_asm_gen.hpp and
mpc_fwd_asm_gen.hpp, the SHA-256 of the whole header under the default knobs and under every knob set the experiment
scripts use, and - default knobs - the SHA-256 of every specialisation by its struct name, so that a mismatch names the
stream that moved.  Hashes only: no generated text.

    python scripts/record_asm_streams.py            # rewrites tests/golden/asm_streams.json
    python scripts/record_asm_streams.py --check    # exit status 1 and the differences if the file would change

tests/test_asm_gen_cpu.py compares against the file through the same functions (KNOB_SETS, generate, hashes).
"""
import hashlib
import importlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chainer_differentiable_mpc_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "asm_streams.json")

GENERATORS = {"lqr_asm_gen.hpp": "gen_lqr_asm", "mpc_fwd_asm_gen.hpp": "gen_mpc_fwd_asm"}

# the knob builds give wrong results on purpose and are never run: they are pinned because scripts/asm_variants.sh,
# build_variants.sh, build_full_variants.sh, fwd_asm_variants.sh and asm_variant_check.sh still use them
KNOB_SETS = {
    "lqr_asm_gen.hpp": [
        {},
        {"GEN_NO_VMWAIT": "1"},
        {"GEN_NO_DMA": "1"},
        {"GEN_NO_LDSREAD": "1"},
        {"GEN_SKIP_FWD": "1"},
        {"GEN_SKIP_BWD": "1"},
        {"GEN_FWD_SKIP": "store,pst,stage,read,xpart,upart"},
        {"GEN_TIMING": "1"},
        {"GEN_NEWTON": "1"},
        {"GEN_WARM_STUBS": "1", "GEN_RET_SETPC": "1"},
        {"GEN_RET_SETPC": "1"},
        {"GEN_MFMA_USE": "4"},
        {"GEN_MFMA_USE": "8", "GEN_MFMA_DEP": "4"},
        {"GEN_QP_VALU": "0"},
        {"GEN_G10_MIX": "1"},
        {"GEN_RING_DEPTH": "4"},
        {"GEN_RING_DEPTH": "5"},
        {"GEN_RING_DEPTH": "6"},
        {"GEN_NT": ""},
        {"GEN_NT": "plain,save,affine,adj,masked,mpc"},
        {"GEN_NO_MFMA": "1"},
        {"GEN_FWD_DEPTH": "12"},
        {"GEN_RING_DEPTH": "4", "GEN_TIMING": "1"},      # the pair the subprocess test sets
    ],
    "mpc_fwd_asm_gen.hpp": [
        {},
        {"GEN_FWD_NO_STORE": "1"},
        {"GEN_FWD_NO_DMA": "1"},
        {"GEN_FWD_NO_LDS": "1"},
        {"GEN_FWD_NO_COST": "1"},
        {"GEN_FWD_NO_ADV": "1"},
        {"GEN_FWD_ROW_MASK": "0"},
        {"GEN_FWD_NT": "1"},
        {"GEN_MFMA_USE": "8"},       # the line-search stream has no matrix instruction: this is its post-label padding
    ],
}

STRUCT = re.compile(r"^(?://[^\n]*\n)?template <>\nstruct ([^\n]+) \{\n.*?^\};\n", re.M | re.S)


def knob_key(env):
    return " ".join("%s=%s" % kv for kv in env.items()) or "default"


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def structs(text):
    """struct name -> text of the specialisation (its summary comment line included)"""
    out = {}
    for m in STRUCT.finditer(text):
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = m.group(0)
    return out


def hashes(text, per_struct):
    h = {"sha256": sha(text)}
    if per_struct:
        h["structs"] = {name: sha(body) for name, body in structs(text).items()}
    return h


def generate(header, env):
    """the header text under the GEN_* variables of `env`, in-process"""
    if CSRC not in sys.path:
        sys.path.insert(0, CSRC)
    gen = importlib.import_module(GENERATORS[header])
    return gen.header_text(gen.Knobs.from_env(env))


def record(generate=generate):
    out = {}
    for header, sets in KNOB_SETS.items():
        out[header] = {"knob_sets": {}}
        for env in sets:
            h = hashes(generate(header, env), per_struct=not env)
            out[header]["knob_sets"][knob_key(env)] = h["sha256"]
            if not env:
                out[header]["structs"] = h["structs"]
    return out


def dump(rec):
    return json.dumps(rec, indent=1, sort_keys=True) + "\n"


def main():
    new = dump(record())
    if "--check" in sys.argv[1:]:
        old = open(GOLDEN).read()
        if old != new:
            a, b = json.loads(old), json.loads(new)
            for header in b:
                for part in ("knob_sets", "structs"):
                    for k in sorted(set(a[header][part]) | set(b[header][part])):
                        if a[header][part].get(k) != b[header][part].get(k):
                            print("differs: %s %s %s" % (header, part, k))
            sys.exit(1)
        print("unchanged:", GOLDEN)
        return
    with open(GOLDEN, "w") as fh:
        fh.write(new)
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main()
