"""CPU checks of the delivery chain's host arithmetic (xd-tts_amd/csrc/delivery_plan.h: which stages run, where the delivered
samples lie, the record tables of the stages' launches, the launch extents of a run of rows), driven by
tests/delivery_plan_test.cpp with plain g++ -- arithmetic that the GPU tests exercise only through the audio it produces."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "delivery_plan_test.cpp")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", CSRC, DRIVER, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_delivery_plan(tmp_path):
    r = _build_and_run(tmp_path, "delivery_plan_test", [])
    assert r.returncode == 0 and r.stdout.decode().split() == ["ok"], r.stderr.decode()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_delivery_plan_under_sanitizers(tmp_path):
    """The stand-alone driver (its own main, host code only) once more with the address and undefined-behaviour sanitizers."""
    r = _build_and_run(tmp_path, "delivery_plan_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and r.stdout.decode().split() == ["ok"] and r.stderr == b"", r.stderr.decode()


def test_delivery_plan_header_needs_no_hip():
    src = _read(os.path.join(CSRC, "delivery_plan.h"))
    assert not re.search(r"#\s*include\s*[<\"](hip/|common\.h|kernels\.h|runtime\.h)", src)
    assert not re.search(r"\b(hip[A-Z]\w*|__device__|__global__|__host__)\b", src)
    assert not re.search(r"\bXDTTS_(OK|ERR_\w+)\b|\bfail\(", src)  # no status codes: the boundary turns the exception into one


def test_the_delivery_arithmetic_lives_in_the_header_alone():
    """The records and their running numbers are built in delivery_plan.h and nowhere else; the delivery order is written once."""
    assert '#include "delivery_plan.h"' in _read(os.path.join(CSRC, "kernels.h"))
    for name in os.listdir(CSRC):
        if name != "delivery_plan.h":
            assert not re.search(r"\bstruct (ResampleUtt|LoudUtt|TileUtt|LimUtt|CompUtt) \{", _read(os.path.join(CSRC, name))), name
    # the request paths and the boundary launch no delivery stage themselves: they go through Delivery
    for name in ("griffinlim_handle.cpp", "magnitude.cpp", "api_griffinlim.cpp", "api_gl_magnitude.cpp", "api_gl_delivery.cpp", "api_synthesize.cpp"):
        src = _read(os.path.join(CSRC, name))
        for launch in ("launch_gl_output_normalise(", "launch_loudness_scale(", "launch_resample(", "launch_compress(", "launch_limit("):
            assert launch not in src, (name, launch)
