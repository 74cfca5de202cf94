"""The persistent decoder's kernels (csrc/decoder_persistent.hip), read from the compiler's assembly: no GPU needed.

Every all-gather edge of a step waits for its last publisher, so nothing that waits may stand behind a publish.  A publish is a
`global_store_dwordx2 ... sc1`; stores count in vmcnt on gfx950, so an `s_waitcnt vmcnt(0)` behind one is a wait for the
write-through store's acknowledgement.  The compiler used to place one behind the energy publish of the attention role and
behind the mel-row publish of the projection role, in front of the deferred column block (32 FMAs per lane) -- and it sank the
column block behind the energy publish past the next gather altogether."""
import os
import re
import subprocess

import pytest

from test_kernel_isa_cpu import PKG, makefile_var

SRC = "decoder_persistent.hip"


def object_flags():
    """The extra flags the Makefile gives this translation unit (`build/a.o build/b.o: CXXFLAGS += ...`)."""
    with open(os.path.join(PKG, "Makefile")) as f:
        m = re.search(r"^build/%s\.o\b.*: CXXFLAGS \+= (.*)$" % re.escape(SRC), f.read(), re.M)
    return m.group(1).split() if m else []


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{template arguments as mangled, e.g. 'Li1ELb0ELb0E': the kernel's lines} of every k_decoder_persistent instantiation."""
    hipcc = makefile_var("HIPCC")
    if not os.path.exists(hipcc):
        pytest.skip("no %s" % hipcc)
    out = str(tmp_path_factory.mktemp("isa") / "decoder_persistent.s")
    subprocess.run([hipcc, "--offload-arch=" + makefile_var("ARCH")] + makefile_var("CXXFLAGS").split() + object_flags()
                   + ["--cuda-device-only", "-S", "-x", "hip", os.path.join(PKG, "csrc", SRC), "-o", out],
                   check=True, capture_output=True, timeout=600)
    with open(out) as f:
        lines = f.read().splitlines()
    found = {}
    for i, ln in enumerate(lines):
        m = re.match(r"_Z\w*20k_decoder_persistentI(\w+?)EEv\w*:", ln)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            found[m.group(1)] = lines[i + 1 : end]
    return found


def directive(body, name):
    vals = [int(ln.split()[1]) for ln in body if ln.strip().startswith(name + " ")]
    assert len(vals) == 1, (name, vals)
    return vals[0]


def fmas_behind_publishes(body):
    """For every publish store in program order: the v_fma / v_fmac instructions between it and the next s_waitcnt that has vmcnt(0)."""
    counts = []
    for i, ln in enumerate(body):
        if re.match(r"\tglobal_store_dwordx2 .* sc1\b", ln):
            n = 0
            for nxt in body[i + 1 :]:
                if re.match(r"\ts_waitcnt\b.*\bvmcnt\(0\)", nxt):
                    break
                n += bool(re.match(r"\tv_fmac?_f32", nxt))
            counts.append(n)
    return counts


def test_every_instantiation_is_built_and_has_no_scratch(kernels):
    """Six instantiations: 1 or 2 chunks, lock-step or skewed (2 chunks only), gate-less or gated.  The kernels hold 136 weight
    registers per lane for the whole launch: no scratch (exact), and at most the 256 VGPRs of a wave of a 512-thread workgroup."""
    assert sorted(kernels) == ["Li1ELb0ELb0E", "Li1ELb0ELb1E", "Li2ELb0ELb0E", "Li2ELb0ELb1E", "Li2ELb1ELb0E", "Li2ELb1ELb1E"]
    for name, body in kernels.items():
        scratch, vgpr = directive(body, ".amdhsa_private_segment_fixed_size"), directive(body, ".amdhsa_next_free_vgpr")
        print("k_decoder_persistent<%s>: %d VGPRs, scratch %d" % (name, vgpr, scratch))
        assert scratch == 0, (name, scratch)
        assert vgpr <= 256, (name, vgpr)


@pytest.mark.parametrize("gate", ["Lb0E", "Lb1E"])
def test_one_chunk_kernel_waits_for_no_store_behind_a_publish(kernels, gate):
    """The lock-step loop of the one-chunk kernel publishes, in program order, h_att, the partial energies, h_dec, the mel rows and
    x.  Behind the energies, h_dec and the mel rows stands a deferred column block: 4 x 4 x 2 = 32 v_fmac per lane (h_dec: two more
    for the folded context columns), all of them ahead of the next full vmcnt wait.  Nothing is deferred behind h_att and x.
    Before the waits were removed the counts were 0, 0, 34, 0, 0.
    (The skewed pair loop keeps its waits: without them it measured 1.9 % slower, DESIGN_NOTES.md.)"""
    counts = fmas_behind_publishes(kernels["Li1ELb0E" + gate])
    print("FMAs between each publish and the next s_waitcnt vmcnt(0):", counts)
    assert len(counts) == 5, counts
    assert counts[1] >= 32 and counts[2] >= 32 and counts[3] >= 32, counts
