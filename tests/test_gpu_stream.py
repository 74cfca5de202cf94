"""The stream stage on the GPU (stream.hip: k_stream_join), everything BIT FOR BIT against tests/stream_ref.py -- every step of
the definition is an exactly rounded fp32 or integer operation, so no tolerance appears anywhere: xdtts_griffinlim_join at the
shapes where the kernel can go wrong (one sample, packs that span several utterances, more records than a tile's LDS cache
holds, an utterance across three tiles, zero-length utterances, last packs of 1, 3 and 15 samples with a guard band), both
load routes, fades, dither, programme level; xdtts_synthesize_document against xdtts_synthesize_sequence; isolation."""
import importlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import loudness_ref as lr
import stream_ref as sr
from conftest import synth_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = (sr.F32_FMT, sr.PCM16, sr.ULAW, sr.ALAW)
GUARD = 64


@pytest.fixture(scope="module")
def voc(pkg):
    v = pkg.create_griffin_lim(iters=12, seed=3)
    yield v
    v.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(pkg, voc, audios, gaps, where, **o):
    """the hook against the restatement in one format, guard band included"""
    got, off, guard = voc.join(audios, gaps, opts=pkg.StreamOpts(**o), guard=GUARD)
    want, woff = sr.join(audios, gaps, o.get("format", 1), o.get("dither", 0), o.get("dither_seed", 0), o.get("fade", 0))
    assert off == woff and got.dtype == want.dtype and got.shape == want.shape, where
    assert np.array_equal(_bits(got), _bits(want)), (where, o, int(np.flatnonzero(_bits(got) != _bits(want))[0]))
    assert np.all(guard == 0xA5), (where, o)


def _tiny(count, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = rng.integers(1, 4, count)
    return [sr.signal(int(v), seed=i) for i, v in enumerate(n)], rng.integers(0, 3, count + 1).tolist()


SHAPES = {
    "one sample": lambda: ([sr.signal(1)], None),
    "small mix": lambda: ([sr.signal(n, seed=n) for n in (1, 2, 7, 15, 16, 17, 33)], [0, 1, 3, 0, 16, 5, 0, 2]),
    "300 tiny": lambda: _tiny(300, 7),           # packs that span several utterances; 300 records > the 64 a tile caches
    "three tiles": lambda: ([sr.signal(2 * 16384 + 999, seed=5)], [37, 41]),   # a G.711 tile is 16384 samples
    "zero length": lambda: ([sr.signal(40, 1), sr.signal(0), sr.signal(0), sr.signal(23, 2), sr.signal(50, 3)], [3, 0, 5, 0, 0, 0]),
    "last pack 1": lambda: ([sr.signal(4097, seed=8)], None),     # 1 sample in the last pack of every format
    "last pack 3": lambda: ([sr.signal(8195, seed=9)], None),     # 3
    "last pack 15": lambda: ([sr.signal(16399, seed=10)], None),  # 3 (fp32), 7 (PCM16), 15 (G.711)
}


@pytest.mark.parametrize("fmt", FORMATS)
def test_hook_at_the_shapes_where_the_kernel_can_go_wrong(pkg, voc, fmt):
    for name, make in SHAPES.items():
        audios, gaps = make()
        _check(pkg, voc, audios, gaps, name, format=fmt)
    assert voc.last_timings()["mel_to_linear_ms"] > 0.0  # ms[0]: the stage alone


@pytest.mark.parametrize("fmt", FORMATS)
def test_both_load_routes_give_the_same_bytes(pkg, voc, fmt):
    """The same utterance read from four host addresses, 0 to 3 floats off a 16-byte boundary: the hook stages it at the same
    phase on the device, so offset 0 takes the 128-bit loads and the others the scalar ones."""
    n = 5000
    base = np.zeros(n + 8, np.float32)
    start = (-(base.ctypes.data // 4)) % 4
    x = sr.signal(n, seed=21)
    want, _ = sr.join([x], [5, 9], fmt, fade=64)
    for a in range(4):
        view = base[start + a:start + a + n]
        view[:] = x
        assert (view.ctypes.data // 4) % 4 == a
        got, _ = voc.join([view], [5, 9], opts=pkg.StreamOpts(format=fmt, fade=64))
        assert np.array_equal(_bits(got), _bits(want)), a


@pytest.mark.parametrize("fade", (1, 5, 64, 4800))
def test_fades(pkg, voc, fade):
    """lengths shorter than, equal to and longer than 2 fade (and odd ones: the middle sample is left alone)"""
    lens = sorted({1, 2, max(fade - 1, 1), fade, 2 * fade - 1, 2 * fade, 2 * fade + 1, 2 * fade + 37})
    audios = [sr.signal(n, seed=n % 13) for n in lens]
    gaps = [(3 * i) % 5 for i in range(len(lens) + 1)]
    for fmt in FORMATS:
        _check(pkg, voc, audios, gaps, ("fade", fade), format=fmt, fade=fade)


def test_dither_is_a_function_of_the_stream_position(pkg, voc):
    x = sr.signal(3000, seed=4)
    a, _ = voc.join([x], [0, 0], opts=pkg.StreamOpts(dither=1, dither_seed=77))
    b, off = voc.join([x], [1234, 0], opts=pkg.StreamOpts(dither=1, dither_seed=77))
    assert off == [1234] and not np.array_equal(a, b[1234:]) and not b[:1234].any()
    assert np.array_equal(a, sr.join([x], [0, 0], sr.PCM16, 1, 77)[0])
    assert np.array_equal(b, sr.join([x], [1234, 0], sr.PCM16, 1, 77)[0])
    plain, _ = voc.join([x])
    assert np.abs(a.astype(np.int32) - plain.astype(np.int32)).max() <= 2  # TPDF of +-1 LSB around the rounded value
    _check(pkg, voc, *SHAPES["300 tiny"](), "dither tiny", dither=1, dither_seed=5, fade=1)


@pytest.mark.parametrize("Q", (22050, 48000))
def test_programme_level(pkg, voc, Q):
    """-16 LUFS / -1 dBTP on about 1.5 s of the loudness tests' signal cut into three utterances with 0.3 s gaps: ONE
    measurement of the level-0 / format-0 stream, ONE gain by the rule, the output = fl(stream gain) encoded."""
    N = int(1.5 * Q)
    x = lr.speech_like(Q, N)
    cuts = [0, N // 3 + 7, 2 * N // 3 - 5, N]
    audios = [np.ascontiguousarray(x[a:b]) for a, b in zip(cuts, cuts[1:])]
    g = int(0.3 * Q)
    gaps = [0, g, g, 0]
    fade = 64
    voc.set_loudness(None)
    with pytest.raises(pkg.XdttsError) as e:   # level 1 without a target
        voc.join(audios, gaps, rate=Q, opts=pkg.StreamOpts(level=1))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG and "target" in str(e.value)
    stream0, _ = voc.join(audios, gaps, opts=pkg.StreamOpts(format=0, fade=fade))
    assert np.array_equal(_bits(stream0), _bits(sr.join(audios, gaps, 0, fade=fade)[0]))
    want = voc.loudness(stream0, Q)
    T, Cdb = -16.0, -1.0
    try:
        voc.set_loudness(T, Cdb)
        for fmt in FORMATS:
            got, _ = voc.join(audios, gaps, rate=Q, opts=pkg.StreamOpts(format=fmt, level=1, fade=fade))
            ls = voc.last_loudness()
            assert len(ls) == 1
            l = ls[0]
            assert (l.mean_square, l.true_peak, l.sample_peak, l.blocks, l.gated_blocks) == \
                   (want.mean_square, want.true_peak, want.sample_peak, want.blocks, want.gated_blocks)
            assert l.gated_blocks > 0
            # the rule, in the double arithmetic of the definition
            gain = 10.0 ** ((T + 0.691) / 20.0) / math.sqrt(l.mean_square)
            if gain * l.true_peak > 10.0 ** (Cdb / 20.0):
                gain = 10.0 ** (Cdb / 20.0) / l.true_peak
            assert l.gain == gain, (l.gain, gain)
            ref = sr.encode(stream0 * np.float32(l.gain), fmt)
            # (the gaps stay exact zeros: +0 times a positive gain)
            assert np.array_equal(_bits(got), _bits(ref)), (Q, fmt)
    finally:
        voc.set_loudness(None)


# ---- xdtts_synthesize_document ---------------------------------------------------------------------------------------------

GAPS = (0, 441, 0, 100)


def _ids():
    return [synth_ids(n, seed=70 + i) for i, n in enumerate([40, 33, 52])]


@pytest.fixture(scope="module")
def seq(pkg, model, voc):
    """the sequence the documents are compared with: computed once"""
    o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
    mels, audios = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o)
    return o, [m.copy() for m in mels], [a.copy() for a in audios]


def test_document_is_the_sequence_joined(pkg, model, voc, seq):
    o, mels, audios = seq
    dm, stream, off = pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(format=0), opts=o)
    want, woff = sr.join(audios, GAPS, 0)
    assert off == woff == pkg.stream_plan([a.size for a in audios], GAPS)[0] and stream.size == pkg.stream_plan([a.size for a in audios], GAPS)[1]
    assert stream.dtype == np.float32 and np.array_equal(_bits(stream), _bits(want))
    for a, b in zip(mels, dm):
        assert a.shape == b.shape and np.array_equal(a, b)
    # the concatenation with zeros in the gaps, written out
    cat = np.concatenate([np.zeros(GAPS[0], np.float32)] + [np.concatenate([a, np.zeros(g, np.float32)]) for a, g in zip(audios, GAPS[1:])])
    assert np.array_equal(stream, cat)
    _m, pcm, _ = pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(format=1), opts=o, want_mels=False)
    assert _m is None and pcm.dtype == np.int16 and np.array_equal(pcm, pkg.audio_to_i16(stream))
    _m, pcm_default, _ = pkg.synthesize_document(model, voc, _ids(), GAPS, None, opts=o, want_mels=False)
    assert np.array_equal(pcm_default, pcm)
    # isolation: the plain sequence on the same handles returns the bits it returned before
    mels2, audios2 = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o)
    for a, b in zip(audios, audios2):
        assert np.array_equal(a, b)
    for a, b in zip(mels, mels2):
        assert np.array_equal(a, b)


def test_document_at_8_khz_in_mu_law(pkg, model, voc, seq):
    o = seq[0]
    voc.set_output_rate(8000)
    try:
        _m, audios = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o, want_mels=False)
        audios = [a.copy() for a in audios]
        _m, stream, off = pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(format=2, fade=40), opts=o, want_mels=False)
    finally:
        voc.set_output_rate(22050)
    want, woff = sr.join(audios, GAPS, sr.ULAW, fade=40)
    assert off == woff and stream.dtype == np.uint8 and np.array_equal(stream, want)


def test_document_with_a_prosody_array(pkg, model, voc, seq):
    o = seq[0]
    pros = [pkg.Prosody(rate=1.25, pitch=1.0), pkg.Prosody(), pkg.Prosody(rate=0.8, pitch=1.1)]
    mels, audios = pkg.synthesize_sequence(model, voc, _ids(), None, opts=o, prosody=pros)
    mels, audios = [m.copy() for m in mels], [a.copy() for a in audios]
    dm, stream, off = pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(format=3), opts=o, prosody=pros)
    want, woff = sr.join(audios, GAPS, sr.ALAW)
    assert off == woff and np.array_equal(stream, want)
    for a, b in zip(mels, dm):
        assert np.array_equal(a, b)


def test_document_at_programme_level(pkg, model, voc, seq):
    """level 1: the utterances enter unlevelled (output_normalise 0, no loudness stage of their own), one struct comes back"""
    o = seq[0]
    raw_voc = pkg.create_griffin_lim(iters=12, seed=3)
    try:
        raw_voc.set_opts(output_normalise=0)
        _m, raw = pkg.synthesize_sequence(model, raw_voc, _ids(), None, opts=o, want_mels=False)
        raw = [a.copy() for a in raw]
    finally:
        raw_voc.close()
    stream0, _ = sr.join(raw, GAPS, 0)
    want = voc.loudness(stream0, 22050)
    try:
        voc.set_loudness(-20.0, -1.0)
        _m, pcm, _ = pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(format=1, level=1), opts=o, want_mels=False)
        ls = voc.last_loudness()
    finally:
        voc.set_loudness(None)
    assert len(ls) == 1 and ls[0].mean_square == want.mean_square and ls[0].true_peak == want.true_peak
    assert np.array_equal(pcm, sr.encode(stream0 * np.float32(ls[0].gain), sr.PCM16))
    with pytest.raises(pkg.XdttsError):   # no target
        pkg.synthesize_document(model, voc, _ids(), GAPS, pkg.StreamOpts(level=1), opts=o)


CHILD = (
    "import sys\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import importlib\n"
    "import torch\n"
    "import numpy as np\n"
    "import oracle\n"
    "import stream_ref as sr\n"
    "from conftest import synth_ids\n"
    "pkg = importlib.import_module('xd-tts_amd')\n"
    "model = pkg.Tacotron2.from_blob(oracle.Oracle('f32').weights_synthetic(seed=20240327, rec_scale=1.0))\n"
    "voc = pkg.create_griffin_lim(iters=12, seed=3)\n"
    "ids = [synth_ids(n, seed=70 + i) for i, n in enumerate([40, 33, 52])]\n"
    "o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)\n"
    "_m, audios = pkg.synthesize_sequence(model, voc, ids, None, opts=o, want_mels=False)\n"
    "audios = [a.copy() for a in audios]\n"
    "_m, pcm, off = pkg.synthesize_document(model, voc, ids, (0, 441, 0, 100), None, opts=o, want_mels=False)\n"
    "want, woff = sr.join(audios, (0, 441, 0, 100), sr.PCM16)\n"
    "assert off == woff and np.array_equal(pcm, want)\n"
    "print('DOCUMENT LAUNCH OK')\n"
)


def test_document_on_the_launch_engines():
    """XDTTS_DECODER=launch and the launch-per-iteration vocoder, in a process of its own: the same document -- the sequence of
    that process, joined."""
    script = CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, XDTTS_DECODER="launch", XDTTS_GL="launch"), capture_output=True,
                       text=True, timeout=300)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "DOCUMENT LAUNCH OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
