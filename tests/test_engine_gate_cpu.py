"""CPU checks of the host-side structure of libxdtts_hip.so: the engines' one fallback policy (xd-tts_amd/csrc/engine_gate.h,
driven by tests/engine_gate_test.cpp with plain g++: the 64-call re-probe no GPU test reaches), and the one place that reads
the environment (csrc/env.cpp) against the list in DESIGN_NOTES.md Appendix B."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")

# removed with the split of api.cpp (spelled without the prefix so that this file passes its own search)
REMOVED = ["LAZY_POLL", "FIRST_POLL", "PFIRST", "XFIRST", "EFIRST", "XLAZY", "CLAZY", "ENC_FIRST", "P8_DELAY", "GL_POLL_DELAY",
           "NO_GRAPH", "NO_SHRINK", "NO_DHEARLY", "DEBUG_MIX", "GEMM_XCD"]


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top):
    if os.path.isfile(top):
        yield top
        return
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x not in ("__pycache__", "build", "build_prof", "golden") and not x.startswith("build_")]
        for n in names:
            if not n.endswith((".so", ".o", ".pyc", ".npy", ".npz", ".bin", ".onnx")):
                yield os.path.join(d, n)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_engine_gate_policy(tmp_path):
    exe = str(tmp_path / "engine_gate_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "engine_gate_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_engine_gate_header_needs_no_hip():
    assert not re.search(r"#\s*include\s*[<\"](hip/|common\.h|kernels\.h|runtime\.h)", _read(os.path.join(CSRC, "engine_gate.h")))


def test_env_cpp_is_the_only_reader_of_the_environment():
    readers = []
    for top in (CSRC, os.path.join(ROOT, "include")):
        for p in _files(top):
            if re.search(r"\bgetenv\b", _read(p)):
                readers.append(os.path.relpath(p, ROOT))
    assert readers == [os.path.join("xd-tts_amd", "csrc", "env.cpp")]


def test_env_table_equals_appendix_b():
    in_code = set(re.findall(r'"(XDTTS_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "env.cpp"))))
    notes = _read(os.path.join(ROOT, "DESIGN_NOTES.md"))
    appendix = notes[notes.index("# Appendix B"):]
    rows = []  # the first table of the appendix: the run-time variables
    for line in appendix.splitlines():
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break
    in_doc = [m for r in rows[2:] for m in re.findall(r"XDTTS_[A-Z0-9_]+", r.split("|")[1])]
    assert len(in_doc) == len(rows) - 2, "one variable per row"
    assert len(set(in_doc)) == len(in_doc)
    assert set(in_doc) == in_code


def test_removed_switches_are_gone():
    hits = []
    pat = re.compile(r"XDTTS_(%s)\b" % "|".join(REMOVED))
    for top in ("xd-tts_amd", "tests", "tools", "bench.py"):
        for p in _files(os.path.join(ROOT, top)):
            if pat.search(_read(p)):
                hits.append(os.path.relpath(p, ROOT))
    assert hits == []
