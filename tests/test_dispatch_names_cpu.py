"""CPU: the names the host dispatch layer is written in stay in step with what mirrors them - the path and family codes of
include/dmpc.h with _lib.py's constants, and the diagnostic switches of csrc/knobs.hpp (the only file in csrc/ that reads the
environment) with INTEGRATION.md's table."""
import glob
import os
import re

from chainer_differentiable_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chainer_differentiable_mpc_amd", "csrc")
KNOBS = os.path.join(CSRC, "knobs.hpp")
# rows of INTEGRATION.md's table that the Python side reads, not the library
PYTHON_SIDE = {"DMPC_LIB", "DMPC_LIB_PARTIAL", "DMPC_SKIP_HASH_CHECK", "DMPC_NO_SAVED_GAINS", "DMPC_NO_DDP_GRAPH",
               "DMPC_PARITY_LOG", "DMPC_BENCH_BACKEND", "DMPC_BENCH_DEVICE"}


def header_enums():
    txt = open(os.path.join(ROOT, "include", "dmpc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: int(v) for body in re.findall(r"\benum\s+dmpc_\w+\s*\{(.*?)\}", txt, flags=re.S)
            for name, v in re.findall(r"\b(DMPC_\w+)\s*=\s*(\d+)", body)}


def test_path_codes_of_the_header_are_the_python_constants():
    enums = header_enums()
    assert len(enums) == 5 + 10 + 3
    for name, value in enums.items():
        assert getattr(_lib, name[len("DMPC_"):]) == value, name
    assert sorted(v for k, v in enums.items() if k.startswith("DMPC_LQR_PATH_")) == list(range(10))
    assert sorted(v for k, v in enums.items() if k.startswith("DMPC_LQR_FAMILY_")) == list(range(1, 6))
    assert sorted(v for k, v in enums.items() if k.startswith("DMPC_F64_PATH_")) == list(range(3))


def test_only_the_switch_header_reads_the_environment():
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
               if "getenv" in open(p).read()]
    assert readers == ["knobs.hpp"]


def test_switch_header_and_integration_table_name_the_same_switches():
    knobs = re.findall(r"^\s*X\((DMPC_[A-Z0-9_]+), (kLatched|kPerCall), -?\d+\)", open(KNOBS).read(), flags=re.M)
    assert len(knobs) == len({n for n, _ in knobs}) == 24
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("## Diagnostics switches"):]
    table = table[:table.index("\n## ")] if "\n## " in table else table
    rows = [line for line in table.splitlines() if line.startswith("| `")]
    documented = {n for line in rows for n in re.findall(r"`(DMPC_[A-Z0-9_]+)", line.split(" | ")[0])}
    assert {n for n, _ in knobs} == documented - PYTHON_SIDE
    # the read mode the table gives is the header's
    per_call = {n for line in rows if "read at every call" in line for n in re.findall(r"`(DMPC_[A-Z0-9_]+)", line)}
    assert per_call == {n for n, mode in knobs if mode == "kPerCall"}
