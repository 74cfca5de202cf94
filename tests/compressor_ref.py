"""fp64 / integer restatement of the dynamic range compressor (include/xdtts.h, "Dynamic range compressor"): the host integers,
the level, the envelope by its SERIAL recurrences (E[n] = max(l[n], E[n - 1] - rho) and the mirror image; the library's device
code uses the closed form by prefix maxima), the gain computer and the output in fp64, the a-priori bounds of an fp32
evaluation, and the inputs the tests use.  numpy only; the CPU tests compare the library's host functions against this, the GPU
tests compare the device against xdtts_compressor_reference."""
import math

import numpy as np

import loudness_ref as lr

LOG10_2 = 0.30102999566398119521
UNIT = 65536
L_FLOOR = -127 * UNIT
SLOPE_MAX = 1 << 18
TILE = 4096
EPS = 2.0 ** -24
RATES = (8000, 22050, 96000)
DB_PER_UNIT = 20.0 * LOG10_2 / UNIT   # dB of one 2^-16 octave
FIELDS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db")
RANGES = {"threshold_db": (-60.0, 0.0), "ratio": (1.0, 20.0), "knee_db": (0.0, 24.0), "attack_ms": (0.1, 100.0), "release_ms": (1.0, 2000.0),
          "makeup_db": (0.0, 24.0)}
DEFAULT = dict(threshold_db=0.0, ratio=1.0, knee_db=0.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
DRC = dict(threshold_db=-24.0, ratio=3.0, knee_db=6.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
# the coefficients the header names (compressor_plan.h: COMP_LOG2_Q, COMP_EXP2_Q), lowest degree first
LOG2_Q = (1.44269502, -0.721339524, 0.480678886, -0.358299077, 0.275221199, -0.19623895, 0.111832075, -0.0419450104, 0.00739540206)
EXP2_Q = (0.693147182, 0.240227208, 0.0554960221, 0.0096521955, 0.00126921665, 0.000208179146)
LOG2_POLY_ERR, EXP2_POLY_ERR = 4e-8, 3e-8   # the header's statements about the two polynomials in exact arithmetic


def settings(**kw):
    """the six fields as the struct holds them: fp32 values, as Python floats"""
    c = dict(DEFAULT)
    c.update(kw)
    return {k: float(np.float32(c[k])) for k in FIELDS}


def _round(v):
    return int(math.floor(v + 0.5))


def slope(ms, Q):
    oct10 = 10.0 / (20.0 * LOG10_2)
    return min(max(_round(65536.0 * oct10 / (ms * float(Q) / 1000.0)), 1), SLOPE_MAX)


def q16(db):
    return _round(db * (65536.0 / (20.0 * LOG10_2)))


def plan(Q, c):
    return {"alpha": slope(c["attack_ms"], Q), "rho": slope(c["release_ms"], Q), "T": q16(c["threshold_db"]), "W": q16(c["knee_db"]), "tile": TILE}


def level(x):
    """l[n] = round(65536 log2 |x[n]|) for normal floats, L_FLOOR for zeros and denormals: int64"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    normal = a >= 2.0 ** -126
    l = np.full(a.shape, L_FLOOR, dtype=np.int64)
    l[normal] = np.floor(65536.0 * np.log2(a[normal]) + 0.5).astype(np.int64)
    return l


# lvl against 65536 log2 |x|:  |f q(f) - log2(1 + f)| <= 4e-8 (the header's statement; test_compressor_cpu recomputes it in
# fp64), eight fmaf roundings of partial Horner values of magnitude <= 1.45 (recomputed there too) and the product's
# rounding, each 2^-24 relative: (4e-8 + 9 * 1.45 * 2^-24 + 2^-24) octaves; times 65536; plus the rounding of 65536 p + 0.5 to
# fp32 (half an ulp of a value up to 65536.5: 2^-8) and the truncation to an integer (0.5).
LVL_BOUND = 0.5 + 2.0 ** -8 + 65536.0 * (LOG2_POLY_ERR + 9 * 1.45 * EPS + EPS)   # 0.562 units
# 2^f, f in [0, 1]: |1 + f q(f) - 2^f| <= 3e-8, five fmaf roundings of partial values <= 0.7, the last fmaf's rounding of a
# value in [1, 2]: relative to 2^f >= 1
EXP2_BOUND = EXP2_POLY_ERR + 5 * 0.7 * EPS + 2 * EPS


def envelope(l, alpha, rho):
    """V from l by the serial recurrences, in Python integers"""
    l = [int(v) for v in l]
    n = len(l)
    V = [0] * n
    e = None
    for i in range(n):
        e = l[i] if e is None else max(l[i], e - rho)
        V[i] = e
    e = None
    for i in range(n - 1, -1, -1):
        e = l[i] if e is None else max(l[i], e - alpha)
        V[i] = max(V[i], e)
    return np.array(V, dtype=np.int64)


def is_identity(c):
    return c["ratio"] == 1.0 and c["makeup_db"] == 0.0


def compress(x, Q, c, l=None):
    """The definition in fp64: dict with out, g (without the make-up), r, o, V, P, engaged, compressed, max_over.  s, mk enter
    as the fp32 values the definition names; l defaults to this file's own level (pass the library's for integer-exact
    comparisons of the envelope and the counts)."""
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.size
    peak = float(np.abs(x64).max()) if n else 0.0
    if is_identity(c) or peak == 0.0:
        return {"out": x64.copy(), "g": np.ones(n), "r": np.zeros(n), "engaged": 0, "compressed": 0, "max_over": 0, "peak": 0.0}
    p = plan(Q, c)
    own = l is None
    l = level(x64) if own else np.asarray(l, dtype=np.int64)
    V = envelope(l, p["alpha"], p["rho"])
    P = int(l.max())
    o = V - (P + p["T"])
    W = p["W"]
    s = float(np.float32(1.0 / c["ratio"] - 1.0))
    mk = float(np.float32(10.0 ** (c["makeup_db"] / 20.0)))
    of = o.astype(np.float64)
    r = s * of
    knee = 2 * np.abs(o) < W
    if W > 0:
        r = np.where(knee, s * (of + W / 2.0) ** 2 / (2.0 * W), r)
    r = np.where(2 * o <= -W, 0.0, r)
    g = np.exp2(r / 65536.0)
    return {"out": x64 * (g * mk), "g": g, "r": r, "o": o, "V": V, "P": P, "engaged": 1, "compressed": int((r < 0).sum()),
            "max_over": int(o.max()), "peak": peak, "mk": mk, "s": s, "plan": p}


def gain_bound(Q, c):
    """|out - out64| <= |out64| B for xdtts_compressor_reference against compress() with this file's OWN level.
    o: the library's l differs from round(65536 log2) by at most 1 (|lvl - 65536 log2| <= LVL_BOUND < 1, this file's rounding
    0.5, both integers), max and the tents are 1-Lipschitz in the sup norm, so V and P differ by at most 1 each: |do| <= 2.
    r: the gain computer's slope is at most |s| (continuous across its branches), so 2 |s| units; its fp32 evaluation rounds
    (float) o (exact below 2^24), h, h h, the product and kq itself: 6 2^-24 |r| with |r| <= |s| max(-T, W / 2) (o <= -T as V <= P).
    g: 2^(dr / 65536) - 1, plus EXP2_BOUND; out: the two products' roundings and mk's."""
    p = plan(Q, c)
    s = abs(1.0 / c["ratio"] - 1.0)
    dr = 2.0 * s + 6 * EPS * s * max(-p["T"], p["W"] / 2.0)
    return math.expm1(math.log(2.0) * dr / 65536.0) + EXP2_BOUND + 3 * EPS


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------

def signal(kind, Q, N, seed=0):
    """fp32, N samples"""
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    k = np.arange(N)
    if kind == "impulses":   # a floor at -50 dB, impulses at both ends, at both sides of the first tile boundary and in between
        x = 0.003 * rng.standard_normal(N)
        for i, v in ((0, 0.9), (N - 1, -0.8), (TILE - 1, 0.7), (TILE, -0.95), (N // 3, 0.5), (N // 2 + 17, -0.6)):
            if 0 <= i < N:
                x[i] = v
    elif kind == "steps":    # loud / quiet / loud / very quiet, each a quarter
        amp = np.choose(np.minimum(4 * k // max(N, 1), 3), [0.8, 0.01, 0.4, 0.0005])
        x = amp * np.where(k % 2 == 0, 1.0, -1.0)
    elif kind == "ramp":     # the level climbs 80 dB over the length, then falls back in a tenth of it
        up = 10.0 ** (-4.0 + 4.0 * k / max(N - 1, 1))
        x = up * np.sin(0.3 * k)
        x[N - N // 10:] *= np.linspace(1.0, 0.0, N // 10) ** 2
    elif kind == "zeros":    # two bursts with exact zeros between them and at both ends
        x = np.zeros(N)
        b = max(N // 8, 1)
        x[b:2 * b] = 0.5 * np.sin(0.2 * np.arange(b))
        x[N - 2 * b:N - b] = 0.9 * rng.standard_normal(b) * 0.3
    elif kind == "speech":
        return lr.speech_like(Q, N, seed)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


KINDS = ("impulses", "steps", "ramp", "zeros", "speech")


def two_level(N, loud=0.5, quiet_db=-40.0, loud_first=True):
    """2 N samples of alternating sign: N at `loud`, N at `quiet_db` under it (or the other way round)"""
    sign = np.where(np.arange(2 * N) % 2 == 0, 1.0, -1.0)
    a = np.concatenate([np.full(N, loud), np.full(N, loud * 10.0 ** (quiet_db / 20.0))])
    if not loud_first:
        a = a[::-1]
    return (a * sign).astype(np.float32)


def block_level_spread(x, Q, ms=400.0, lo=10.0, hi=95.0):
    """the spread in dB between the hi-th and lo-th percentile of the rms levels of consecutive blocks (digital silence left out)"""
    x = np.asarray(x, dtype=np.float64)
    b = int(Q * ms / 1000.0)
    lv = []
    for i in range(0, x.size - b + 1, b):
        ms2 = float(np.mean(x[i:i + b] ** 2))
        if ms2 > 0.0:
            lv.append(10.0 * math.log10(ms2))
    return float(np.percentile(lv, hi) - np.percentile(lv, lo))
