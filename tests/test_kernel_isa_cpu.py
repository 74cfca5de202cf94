"""Code size of the two kernels of the batched two-launch decoder, read from the compiler's assembly: no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "xd-tts_amd")


def makefile_var(name):
    """`NAME ?= value` of the library's Makefile (the environment wins, as it does for make)."""
    with open(os.path.join(PKG, "Makefile")) as f:
        value = re.search(r"^%s \?= (.*)$" % name, f.read(), re.M).group(1)
    return os.environ.get(name, value)


def kernel_stats(asm, mangled_part):
    """(instruction lines, .private_segment_fixed_size) of the one kernel whose mangled name contains `mangled_part`.
    An instruction line lies between the kernel's label and its .Lfunc_end, starts with a tab and a lower-case letter
    and is not a directive (directives start with a dot)."""
    lines = asm.splitlines()
    starts = [i for i, ln in enumerate(lines) if re.match(r"_Z\w*%s\w*:" % re.escape(mangled_part), ln)]
    assert len(starts) == 1, (mangled_part, len(starts))
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[starts[0] + 1 : end]
    scratch = [int(ln.split()[1]) for ln in body if ln.strip().startswith(".amdhsa_private_segment_fixed_size")]
    assert len(scratch) == 1, (mangled_part, scratch)
    return sum(1 for ln in body if re.match(r"\t[a-z]", ln)), scratch[0]


def test_two_launch_kernels_keep_their_code_size(tmp_path):
    """Round 6 left three rejected rebuilds inside the default instantiations of these kernels as run-time branches: the attention
    launch grew 8.4x (about 130 kB of code against a 64 kB instruction cache), the decoder-LSTM launch by 40 %, and no parity test or
    perf guard noticed.  The reference counts are those of decoder.hip as of commit 44bacef (the last one before the rebuilds),
    compiled against this tree's headers with this function's rule by AMD clang 22.0.0git (roc-7.2.0, HIP 7.2.26015):
    k_att_lstm_attention<true,true> 4012, k_lstm_mfma<2560,1> 13926.  10 % above them leaves room for a compiler point release and
    small honest edits.  Neither kernel has scratch, which is an exact condition."""
    hipcc = makefile_var("HIPCC")
    if not os.path.exists(hipcc):
        pytest.skip("no %s" % hipcc)
    out = str(tmp_path / "decoder.s")
    subprocess.run([hipcc, "--offload-arch=" + makefile_var("ARCH")] + makefile_var("CXXFLAGS").split()
                   + ["--cuda-device-only", "-S", "-x", "hip", os.path.join(PKG, "csrc", "decoder.hip"), "-o", out],
                   check=True, capture_output=True, timeout=600)
    with open(out) as f:
        asm = f.read()
    for part, reference in (("k_att_lstm_attentionILb1ELb1E", 4012), ("k_lstm_mfmaILi2560ELi1E", 13926)):
        count, scratch = kernel_stats(asm, part)
        print("%s: %d instructions (reference %d), scratch %d" % (part, count, reference, scratch))
        assert scratch == 0, (part, scratch)
        assert count <= 1.10 * reference, (part, count, reference)
