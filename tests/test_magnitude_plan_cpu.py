"""CPU checks of the magnitude chain's host arithmetic (xd-tts_amd/csrc/magnitude_plan.h: what a request asks for, which stages
run, the frames behind them, the record tables of the stages' launches, the buffer the loop reads), driven by
tests/magnitude_plan_test.cpp with plain g++ -- arithmetic that the GPU tests exercise only through the audio it produces."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "magnitude_plan_test.cpp")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", CSRC, DRIVER, "-o", exe])
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_magnitude_plan(tmp_path):
    r = _build_and_run(tmp_path, "magnitude_plan_test", [])
    assert r.returncode == 0 and r.stdout.decode().split() == ["ok"], r.stderr.decode()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_magnitude_plan_under_sanitizers(tmp_path):
    """The stand-alone driver (its own main, host code only) once more with the address and undefined-behaviour sanitizers."""
    r = _build_and_run(tmp_path, "magnitude_plan_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0 and r.stdout.decode().split() == ["ok"] and r.stderr == b"", r.stderr.decode()


def test_magnitude_plan_header_needs_no_hip():
    src = _read(os.path.join(CSRC, "magnitude_plan.h"))
    assert not re.search(r"#\s*include\s*[<\"](hip/|common\.h|kernels\.h|runtime\.h|xdtts\.h)", src)
    assert not re.search(r"\b(hip[A-Z]\w*|__device__|__global__|__host__)\b", src)
    assert not re.search(r"\bXDTTS_(OK|ERR_\w+)\b|\bfail\(", src)  # no status codes: the boundary turns the exception into one


def test_the_magnitude_arithmetic_lives_in_the_header_alone():
    """The records are defined in magnitude_plan.h and nowhere else; the magnitude order is written once, in magnitude.cpp."""
    assert '#include "magnitude_plan.h"' in _read(os.path.join(CSRC, "kernels.h"))
    records = r"\bstruct (ProsodyUtt|ContourUtt|TimbreUtt|F0Utt|SpsiSeg|SpsiUtt) \{"
    assert len(re.findall(records, _read(os.path.join(CSRC, "magnitude_plan.h")))) == 6
    for name in os.listdir(CSRC):
        if name != "magnitude_plan.h":
            assert not re.search(records, _read(os.path.join(CSRC, name))), name
    # the request paths and the boundary launch no magnitude stage themselves: they go through Magnitude
    for name in ("griffinlim_handle.cpp", "api_griffinlim.cpp", "api_gl_magnitude.cpp", "api_gl_delivery.cpp", "api_synthesize.cpp"):
        src = _read(os.path.join(CSRC, name))
        for launch in ("launch_prosody(", "launch_prosody_batch(", "launch_prosody_contour(", "launch_timbre(", "launch_f0_frames(", "launch_f0_track(",
                       "launch_spsi("):
            assert launch not in src, (name, launch)
