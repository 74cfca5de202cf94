"""CPU checks of the vocoder's host arithmetic (xd-tts_amd/csrc/gl_plan.h: the single call's split, the ragged-rows table and the
batch packing plan), driven by tests/gl_plan_test.cpp with plain g++: CU counts, workgroups per CU and forced shapes that the GPU
tests, which run on one device, never reach."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gl_plan(tmp_path):
    exe = str(tmp_path / "gl_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "gl_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_gl_plan_header_needs_no_hip():
    src = _read(os.path.join(CSRC, "gl_plan.h"))
    assert not re.search(r"#\s*include\s*[<\"](hip/|common\.h|kernels\.h|runtime\.h)", src)
    assert not re.search(r"\b(hip[A-Z]\w*|__device__|__global__|__host__)\b", src)


def test_the_plan_lives_in_the_header_alone():
    assert '#include "gl_plan.h"' in _read(os.path.join(CSRC, "kernels.h"))
    for name in os.listdir(CSRC):
        if name != "gl_plan.h":
            src = _read(os.path.join(CSRC, name))
            assert not re.search(r"\bbool gl_persistent_plan\(|\bstruct GlSeg\b|\bstruct AnRows\b|gl_run_from_device_mel_prosody", src), name
