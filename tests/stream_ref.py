"""The stream stage restated in numpy, independently of csrc/stream_plan.h: offsets and total, the fade, the fp32 step order,
the Rust cast, the TPDF dither and both G.711 laws (include/xdtts.h: the definition above xdtts_stream_opts).  Every fp32
step is one numpy float32 operation, i.e. rounded on its own.  G.711 is written another way than the header's bit formulas:
a searchsorted over each law's segment thresholds, and a decoder table per law."""
import math

import numpy as np

F32 = np.float32
F32_FMT, PCM16, ULAW, ALAW = 0, 1, 2, 3
DTYPE = {F32_FMT: np.float32, PCM16: np.dtype("<i2"), ULAW: np.uint8, ALAW: np.uint8}
SILENCE = {F32_FMT: 0.0, PCM16: 0, ULAW: 0xFF, ALAW: 0xD5}
DITHER_STREAM = 0x57AEA401
UTT_MAX, FADE_MAX, TOTAL_MAX = 4096, 4800, 1 << 28
M32 = np.uint64(0xFFFFFFFF)


# ---- the counter-based generator (the specification the oracle shares) ----------------------------------------------------

def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def rng_uniform(seed, stream, idx):
    a = _mix32(np.uint64((int(seed) ^ 0x9E3779B9) & 0xFFFFFFFF))
    b = _mix32((a + np.uint64(stream)) & M32)
    u = _mix32((b + (np.asarray(idx, dtype=np.uint64) & M32)) & M32)
    return (u >> np.uint64(8)).astype(np.float32) * F32(1.0 / 16777216.0)


def dither(seed, k):
    k = np.asarray(k, dtype=np.uint64)
    return rng_uniform(seed, DITHER_STREAM, 2 * k) - rng_uniform(seed, DITHER_STREAM, 2 * k + 1)


# ---- layout ------------------------------------------------------------------------------------------------------------------

def plan(n, gaps=None):
    """(offsets, total) in Python integers; ValueError where the rules of the layout refuse."""
    U = len(n)
    if not 1 <= U <= UTT_MAX:
        raise ValueError("n_utt")
    g = [0] * (U + 1) if gaps is None else [int(v) for v in gaps]
    at, off = g[0], []
    for u in range(U):
        off.append(at)
        at += int(n[u]) + g[u + 1]
    if not 1 <= at < TOTAL_MAX:
        raise ValueError("total")
    return off, at


def fade_table(fade):
    # (math.cos: the C library's, as the host computes it; the product pi (j + 0.5) is formed first, then divided)
    return np.array([0.5 - 0.5 * math.cos(math.pi * (j + 0.5) / fade) for j in range(fade)], dtype=np.float64).astype(np.float32)


# ---- one sample -----------------------------------------------------------------------------------------------------------------

def cast_i16(v):
    """Rust's `v as i16` on float32: truncation toward zero, saturation, NaN -> 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.clip(np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=1e9, neginf=-1e9), -32768.0, 32767.0))
    return t.astype(np.int32)


def quantise(x, dither_on=0, seed=0, k=None):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * F32(32767.0)
        if not dither_on:
            return cast_i16(v)
        v = v + dither(seed, k)
        r = np.floor(v + F32(0.5))
    r = np.clip(np.nan_to_num(r.astype(np.float64), nan=0.0, posinf=1e9, neginf=-1e9), -32768.0, 32767.0)
    return r.astype(np.int32)


_ULAW_EDGES = np.array([64, 128, 256, 512, 1024, 2048, 4096], dtype=np.int64)   # biased 14-bit magnitude: where a segment begins
_ALAW_EDGES = np.array([32, 64, 128, 256, 512, 1024, 2048], dtype=np.int64)     # 12-bit magnitude


def ulaw(q):
    q = np.asarray(q, dtype=np.int64)
    a = np.minimum(np.abs(q), 32767)
    m = np.minimum(a // 4, 8158) + 33
    e = np.searchsorted(_ULAW_EDGES, m, side="right")
    mant = (m - (np.int64(32) << e)) // (np.int64(2) << e)
    return (0xFF ^ (np.where(q < 0, 0x80, 0) | (e << 4) | mant)).astype(np.uint8)


def alaw(q):
    q = np.asarray(q, dtype=np.int64)
    a13 = np.minimum(np.abs(q), 32767) // 8
    e = np.searchsorted(_ALAW_EDGES, a13, side="right")
    mant = np.where(e == 0, a13 // 2, (a13 >> e) - 16)
    return ((np.where(q < 0, 0, 0x80) | (e << 4) | mant) ^ 0x55).astype(np.uint8)


def ulaw_table():
    """byte -> 16-bit linear, the common decoder: ((mant << 3) + 132 << e) - 132, negated where the sign bit is set"""
    b = 0xFF ^ np.arange(256, dtype=np.int64)
    t = ((((b & 15) << 3) + 132) << ((b >> 4) & 7)) - 132
    return np.where(b & 0x80, -t, t)


def alaw_table():
    b = np.arange(256, dtype=np.int64) ^ 0x55
    e, mant = (b >> 4) & 7, b & 15
    t = np.where(e == 0, (mant << 4) + 8, ((mant << 4) + 0x108) << np.maximum(e - 1, 0))
    return np.where(b & 0x80, t, -t)


def encode(x, fmt, dither_on=0, seed=0, k=None):
    """steps 3 to 5 on samples behind fade and gain, at stream positions k"""
    x = np.asarray(x, dtype=np.float32)
    if fmt == F32_FMT:
        return x.copy()
    if fmt == PCM16:
        return quantise(x, dither_on, seed, k).astype(DTYPE[PCM16])
    q = quantise(x)
    return ulaw(q) if fmt == ULAW else alaw(q)


# ---- the stream ----------------------------------------------------------------------------------------------------------------

def shape(x, fade=0, gain=None):
    """steps 1 and 2 on one utterance"""
    y = np.array(x, dtype=np.float32)
    n = y.size
    f = min(int(fade), n // 2)
    if f > 0:
        T = fade_table(int(fade))[:f]
        y[:f] = y[:f] * T
        y[n - f:] = y[n - f:] * T[::-1]
    if gain is not None:
        y = y * F32(gain)
    return y


def join(audios, gaps=None, fmt=PCM16, dither_on=0, seed=0, fade=0, gain=None):
    """The stream of the definition: (array of DTYPE[fmt], offsets)."""
    off, total = plan([len(a) for a in audios], gaps)
    out = np.full(total, SILENCE[fmt], dtype=DTYPE[fmt])
    for a, o in zip(audios, off):
        if len(a):
            out[o:o + len(a)] = encode(shape(a, fade, gain), fmt, dither_on, seed, np.arange(o, o + len(a)))
    return out, off


def signal(n, seed=0, scale=0.9):
    """test input: a few sines under an envelope plus noise, in (-1, 1), with exact zeros nowhere special"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * np.sin(2 * np.pi * t / 37.3) + 0.3 * np.sin(2 * np.pi * t / 5.1 + 1.0) + 0.2 * rng.standard_normal(n)
    return (scale * x / max(1.0, np.abs(x).max() if n else 1.0)).astype(np.float32)
