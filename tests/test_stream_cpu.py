"""The stream stage without a GPU: the bindings; both G.711 laws over all 65 536 values of q against the restatement, against
`audioop` for q >= 0, their mirror symmetry and their decode error; the PCM16 cast against xdtts_audio_to_i16; the TPDF
dither's range, mean and variance; the plan and the fade table bit for bit; every argument error as a status code before a
device is touched; the stand-alone driver of stream_plan.h under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
NEW = ("xdtts_stream_opts_default", "xdtts_stream_sample_bytes", "xdtts_stream_plan", "xdtts_stream_fade_table",
       "xdtts_stream_encode_sample", "xdtts_griffinlim_join", "xdtts_synthesize_document")
Q_ALL = np.arange(-32768, 32768, dtype=np.int64)


def test_symbols_are_declared_exported_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "xdtts.h")).read()
    raw = C.CDLL(pkg.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in pkg.SYMBOLS, name
    assert callable(pkg.GriffinLim.join) and callable(pkg.synthesize_document)
    assert C.sizeof(pkg.StreamOpts) == 20 and re.search(r"}\s*xdtts_stream_opts\s*;", header)
    o = pkg.StreamOpts()
    assert (o.format, o.dither, o.dither_seed, o.level, o.fade) == (1, 0, 0, 0, 0)
    assert [pkg.stream_sample_bytes(f) for f in (0, 1, 2, 3, 4, -1)] == [4, 2, 1, 1, 0, 0]
    assert "0x57AEA401" in header and "%#X" % sr.DITHER_STREAM == "0X57AEA401"


def _x_of_q(q):
    """a float32 whose undithered q of step 4 is q: fl(x 32767) truncates to q"""
    x = ((np.asarray(q, dtype=np.float64) + np.where(np.asarray(q) >= 0, 0.25, -0.25)) / 32767.0).astype(np.float32)
    assert np.array_equal(sr.quantise(x), np.clip(q, -32768, 32767))
    return x


@pytest.fixture(scope="module")
def g711(pkg):
    """xdtts_stream_encode_sample over all 65 536 q, both laws: computed once"""
    x = _x_of_q(Q_ALL)
    x[0] = np.float32(-1.5)  # q = -32768 is reached by saturation only
    assert sr.quantise(x)[0] == -32768
    out = {}
    for fmt in (sr.ULAW, sr.ALAW):
        out[fmt] = np.array([pkg.stream_encode_sample(v, fmt) for v in x], dtype=np.uint8)
    return out


@pytest.mark.parametrize("fmt", [sr.ULAW, sr.ALAW])
def test_g711_equals_the_restatement_over_all_q(g711, fmt):
    ref = sr.ulaw(Q_ALL) if fmt == sr.ULAW else sr.alaw(Q_ALL)
    assert np.array_equal(g711[fmt], ref)


@pytest.mark.parametrize("fmt", [sr.ULAW, sr.ALAW])
def test_g711_equals_audioop_for_non_negative_q(g711, fmt):
    audioop = pytest.importorskip("audioop")
    pos = Q_ALL[Q_ALL >= 0]
    raw = pos.astype("<i2").tobytes()
    theirs = np.frombuffer(audioop.lin2ulaw(raw, 2) if fmt == sr.ULAW else audioop.lin2alaw(raw, 2), dtype=np.uint8)
    assert np.array_equal(g711[fmt][Q_ALL >= 0], theirs)


@pytest.mark.parametrize("fmt,bound", [(sr.ULAW, 644), (sr.ALAW, 512)])
def test_g711_mirror_and_decode_error(g711, fmt, bound):
    enc = dict(zip(Q_ALL.tolist(), g711[fmt].tolist()))
    for q in range(1, 32768):
        assert enc[-q] == enc[q] ^ 0x80, q
    assert enc[-32768] == enc[32767] ^ 0x80
    table = sr.ulaw_table() if fmt == sr.ULAW else sr.alaw_table()
    err = np.abs(table[g711[fmt]] - Q_ALL)
    assert err.max() == bound and err[0] == bound  # the maximum is reached at q = -32768


def test_pcm16_without_dither_is_audio_to_i16(pkg):
    steps = (np.arange(-40, 41, dtype=np.float64) + 0.5) / 32767.0
    edge = np.concatenate([steps * (1 - 1e-6), steps, steps * (1 + 1e-6), (np.arange(-5, 6) * 1000 + 0.5) / 32767.0])
    x = np.concatenate([np.array([1.0, -1.0, 1.00001, -1.00001, np.nan, np.inf, -np.inf, 0.0, -0.0, 0.999985, 3.0e-5, -3.0e-5], np.float64), edge]).astype(np.float32)
    want = pkg.audio_to_i16(x)
    got = np.array([pkg.stream_encode_sample(v, sr.PCM16) for v in x], dtype=np.int16)
    assert np.array_equal(got, want) and np.array_equal(sr.encode(x, sr.PCM16), want)
    # format 0 keeps the bits, the sign of zero and a NaN's payload included
    got0 = np.array([pkg.stream_encode_sample(v, 0) for v in x], dtype=np.float32)
    assert np.array_equal(got0.view(np.uint32), x.view(np.uint32))


def test_tpdf_dither_range_mean_variance_and_parity(pkg):
    n = 1 << 16
    k = np.arange(n)
    d = sr.dither(99, k).astype(np.float64)
    assert d.min() > -1.0 and d.max() < 1.0
    assert abs(d.mean()) <= 4.0 / np.sqrt(6.0 * n)   # four standard errors of a triangular variable (variance 1/6)
    assert abs(d.var() - 1.0 / 6.0) <= 0.05 / 6.0
    # the library's dither is the restatement's: the encoded values agree on arbitrary samples
    x = sr.signal(4096, seed=3)
    kk = np.arange(5000, 5000 + x.size)
    got = np.array([pkg.stream_encode_sample(v, sr.PCM16, 1, 99, int(i)) for v, i in zip(x, kk)], dtype=np.int16)
    assert np.array_equal(got, sr.encode(x, sr.PCM16, 1, 99, kk))
    assert not np.array_equal(got, sr.encode(x, sr.PCM16, 1, 99, kk + 1))   # a function of the absolute position
    assert not np.array_equal(got, sr.encode(x, sr.PCM16, 1, 100, kk))      # ... and of the seed
    # saturation and NaN with dither on
    for v, want in ((2.0, 32767), (-2.0, -32768), (float("nan"), 0), (float("inf"), 32767), (float("-inf"), -32768)):
        assert pkg.stream_encode_sample(v, sr.PCM16, 1, 5, 17) == want


def test_plan_and_fade_table_equal_the_restatement_bit_for_bit(pkg):
    rng = np.random.Generator(np.random.PCG64(4))
    cases = [([1], None), ([1, 2, 7, 15, 16, 17, 33], [0, 1, 3, 0, 16, 5, 0, 2]), ([0, 0, 5], [1, 0, 0, 0]), ([(1 << 28) - 2], [0, 1])]
    for _ in range(20):
        U = int(rng.integers(1, 40))
        cases.append((rng.integers(0, 5000, U).tolist(), rng.integers(0, 3000, U + 1).tolist()))
    for n, gaps in cases:
        assert pkg.stream_plan(n, gaps) == sr.plan(n, gaps), (n, gaps)
    assert pkg.stream_plan([1] * 4096)[1] == 4096
    for fade in (1, 2, 5, 64, 441, 4800):
        ours, ref = pkg.stream_fade_table(fade), sr.fade_table(fade)
        assert ours.dtype == np.float32 and np.array_equal(ours.view(np.uint32), ref.view(np.uint32)), fade
        assert np.all(np.diff(ours) > 0) and 0.0 < ours[0] and ours[-1] <= 1.0
    assert pkg.stream_fade_table(0).size == 0


def test_argument_errors_come_back_without_a_device(pkg):
    lib, BAD = pkg.lib, pkg.XDTTS_ERR_BAD_ARG
    x = np.zeros(8, np.float32)
    out = np.zeros(64, np.uint8)
    tot = C.c_size_t(7)

    def join(n, gaps=None, opts=None, U=None, cap=64):
        U = len(n) if U is None else U
        ns = (C.c_size_t * max(len(n), 1))(*n)
        ip = (C.c_void_p * max(len(n), 1))(*[x.ctypes.data] * len(n))
        gp = None if gaps is None else (C.c_size_t * len(gaps))(*gaps)
        st = lib.xdtts_griffinlim_join(None, ip, ns, U, gp, 22050, C.byref(opts) if opts is not None else None, out.ctypes.data, cap, None, C.byref(tot))
        return st, lib.xdtts_last_error().decode()

    st, msg = join([], U=0)
    assert st == BAD and "n_utt 0" in msg and tot.value == 0
    st, msg = join([1] * 4097)
    assert st == BAD and "n_utt 4097" in msg
    st, msg = join([0, 0], [0, 0, 0])
    assert st == BAD and "total is 0" in msg
    st, msg = join([(1 << 28) - 1, 1])
    assert st == BAD and "n[1]" in msg and "2^28" in msg
    st, msg = join([4], [0, 1 << 28])
    assert st == BAD and "gaps[1]" in msg
    st, msg = join([4], opts=pkg.StreamOpts(fade=4801))
    assert st == BAD and "fade 4801" in msg
    st, msg = join([4], opts=pkg.StreamOpts(format=2, dither=1))
    assert st == BAD and "dither" in msg and "format" in msg
    st, msg = join([4], opts=pkg.StreamOpts(format=4))
    assert st == BAD and "format 4" in msg
    st, msg = join([4], opts=pkg.StreamOpts(level=2))
    assert st == BAD and "level 2" in msg
    st, msg = join([8], opts=pkg.StreamOpts(format=0), cap=31)
    assert st == BAD and "cap_bytes 31" in msg
    st, msg = join([8], opts=pkg.StreamOpts(level=1))  # the rate and the options pass; no handle
    assert st == BAD and "null" in msg
    # the host functions
    with pytest.raises(pkg.XdttsError):
        pkg.stream_plan([])
    with pytest.raises(pkg.XdttsError):
        pkg.stream_plan([1] * 4097)
    with pytest.raises(pkg.XdttsError):
        pkg.stream_plan([0], [0, 0])
    with pytest.raises(pkg.XdttsError):
        pkg.stream_plan([1 << 27, 1 << 27])
    assert pkg.stream_plan([(1 << 27) - 1, 1 << 27])[1] == (1 << 28) - 1
    with pytest.raises(pkg.XdttsError):
        pkg.stream_fade_table(4801)
    for fmt, dith in ((4, 0), (2, 1), (3, 1), (0, 1)):
        with pytest.raises(pkg.XdttsError):
            pkg.stream_encode_sample(0.5, fmt, dith)
    # the document entry: options, count and gaps before a handle is looked at
    nf, total, stream = (C.c_size_t * 1)(), C.c_size_t(), C.c_void_p()
    o = pkg.StreamOpts(format=2, dither=1)
    doc = lib.xdtts_synthesize_document
    assert doc(None, None, None, None, None, None, 1, None, None, None, C.byref(o), None, nf, C.byref(stream), None, C.byref(total)) == BAD
    assert b"dither" in lib.xdtts_last_error()
    assert doc(None, None, None, None, None, None, 0, None, None, None, None, None, nf, C.byref(stream), None, C.byref(total)) == BAD
    assert b"n_utt 0" in lib.xdtts_last_error()
    gp = (C.c_size_t * 2)(0, 1 << 28)
    assert doc(None, None, None, None, None, None, 1, None, None, gp, None, None, nf, C.byref(stream), None, C.byref(total)) == BAD
    assert b"gaps[1]" in lib.xdtts_last_error()
    assert doc(None, None, None, None, None, None, 1, None, None, None, None, None, nf, C.byref(stream), None, C.byref(total)) == BAD
    assert b"null" in lib.xdtts_last_error() and not stream.value


def test_restatement_join_known_answer():
    a = [np.array([0.5, -0.5], np.float32), np.zeros(0, np.float32), np.array([1.0], np.float32)]
    s, off = sr.join(a, [1, 0, 2, 1], sr.PCM16)
    assert off == [1, 3, 5] and s.tolist() == [0, 16383, -16383, 0, 0, 32767, 0]
    s, _ = sr.join(a, [1, 0, 2, 1], sr.ULAW)
    assert s[0] == 0xFF and s[3] == 0xFF and s[5] == 0x80
    s, _ = sr.join(a, [1, 0, 2, 1], sr.ALAW)
    assert s[0] == 0xD5 and s[5] == 0xAA
    # a fade on an utterance shorter than 2 fade: the first f entries only, symmetric
    y = sr.shape(np.ones(5, np.float32), fade=4)
    T = sr.fade_table(4)
    assert y.tolist() == [T[0], T[1], 1.0, T[1], T[0]]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_stream_plan_driver_under_sanitizers(tmp_path):
    """tests/stream_plan_test.cpp with plain g++ and -fsanitize=address,undefined: the plan, the argument rules and the kernel's
    tile / cache / pack walk on the host with every index checked against the sample-by-sample definition."""
    exe = str(tmp_path / "stream_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "stream_plan_test.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok"]


def test_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "stream_plan.h"), encoding="utf-8").read()
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", src) == ["rng.h"]
    assert not re.search(r"#\s*include\s*<hip/", src)
    rng = open(os.path.join(CSRC, "rng.h"), encoding="utf-8").read()
    assert not re.search(r"#\s*include\s*[<\"](hip/|common)", rng)
