"""fp64 restatement of the look-ahead true-peak limiter (include/xdtts.h, "Look-ahead true-peak limiter"): the half width, the
window, the peak envelope, needed gain, hold, smoothing and output, the a-priori bound of an fp32 evaluation, and the inputs the
tests use.  numpy only, on top of loudness_ref.py; the CPU tests compare xdtts_limiter_reference against this, the GPU tests
compare the device against xdtts_limiter_reference."""
import numpy as np

import loudness_ref as lr
from resample_ref import bound

RATES = lr.RATES
GPU_RATES = (8000, 22050, 96000)
LOOKAHEADS = (500, 5000, 10000)
TILE = 4096
EPS = 2.0 ** -24


def half_width(Q, us):
    return max(12, (int(Q) * int(us) + 500000) // 1000000)


def window(H):
    """w[j + H], j = -H .. H, in double: (0.5 + 0.5 cos(pi j / (H + 1))) / (H + 1).  The exact weights sum to 1."""
    j = np.arange(-H, H + 1, dtype=np.float64)
    return (0.5 + 0.5 * np.cos(np.pi * j / (H + 1))) / (H + 1)


def taps32():
    """the loudness stage's true-peak taps as the library holds them: double, rounded once to fp32"""
    return lr.true_peak_taps().astype(np.float32).astype(np.float64)


def envelope(x):
    """(e, A): e[n] = max(|x[n]|, Y[n], Y[n - 1]) with Y[-1] = 0, and A[n] = the largest sum |t| |x| behind any value e[n] is the
    maximum of (what the a-priori error of an fp32 evaluation is proportional to)."""
    x = np.asarray(x, dtype=np.float64)
    t = taps32()
    xp = np.concatenate([np.zeros(12), x, np.zeros(12)])
    win = np.lib.stride_tricks.sliding_window_view(xp, 24)[1:x.size + 1, ::-1]   # x[n - j], j = -12 .. 11
    Y = np.abs(win @ t.T).max(axis=1)
    A = (np.abs(win) @ np.abs(t).T).max(axis=1)
    Yb = np.concatenate([[0.0], Y[:-1]])
    Ab = np.concatenate([[0.0], A[:-1]])
    return np.maximum(np.abs(x), np.maximum(Y, Yb)), np.maximum(A, Ab)


def sliding_min(r, H):
    """m[k], k = -H .. N - 1 + H (index k + H): min r[k - H .. k + H], r = 1 outside"""
    rp = np.concatenate([np.ones(2 * H), r, np.ones(2 * H)])
    return np.lib.stride_tricks.sliding_window_view(rp, 2 * H + 1).min(axis=1)


def limit(x, Q, g0, c, us, w=None):
    """The definition in fp64: dict with out, g, r, e, H, min_gain, limited.  G and c enter as the fp32 values the definition
    names ((float) g0, (float) c); w defaults to the double window rounded once to fp32."""
    x = np.asarray(x, dtype=np.float64)
    H = half_width(Q, us)
    G, cf = float(np.float32(g0)), float(np.float32(c))
    w = window(H).astype(np.float32).astype(np.float64) if w is None else np.asarray(w, dtype=np.float64)
    e, _ = envelope(x)
    a = G * e
    r = np.ones_like(a)
    over = a > cf
    r[over] = cf / a[over]
    m = sliding_min(r, H)                      # N + 2 H values
    d = 1.0 - m
    s = 1.0 - np.lib.stride_tricks.sliding_window_view(d, 2 * H + 1) @ w
    g = np.minimum(s, r)
    return {"out": x * (G * g), "g": g, "r": r, "e": e, "H": H, "min_gain": float(g.min()) if g.size else 1.0,
            "limited": int((g < 1.0).sum())}


def gain_bound(x, Q, g0, c, us):
    """|g - g64| <= (26 S G max|x| / c + 2 H + 12) 2^-24, S = max_p sum_j |t[4 j + p]|: the peak evaluation (resample_ref.bound's
    rule, 26 2^-24 sum |t| |x| <= 26 2^-24 S max|x|) scaled by G / c, through r (1-Lipschitz in a / c above the threshold,
    continuous at it), min and the weighted average (1-Lipschitz), plus the chain's 2 H + 1 roundings of a sum <= 1 and the
    roundings of a, r, d, s and the window's weights (the 12)."""
    S = float(np.abs(taps32()).sum(axis=1).max())
    G, cf = float(np.float32(g0)), float(np.float32(c))
    H = half_width(Q, us)
    return (26.0 * S * G * float(np.abs(x).max()) / cf + 2 * H + 12) * EPS


def delivered_lufs(y, Q):
    return lr.measure(y, Q)["lufs"]


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------

def lengths(Q, us):
    H = half_width(Q, us)
    return (1, H, 2 * H + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2 * H + 5)


def signal(Q, us, N, seed=0):
    """fp32, N samples: a noise floor at -40 dB carrying an impulse at 0 and at N - 1, impulses at TILE - 1 and TILE, two peaks
    2 H - 1 apart and two peaks 4 H + 2 apart, a plateau longer than 2 H + 1, and a quarter-rate burst (its peak lies between the
    samples) -- each only where N has room for it."""
    H = half_width(Q, us)
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    x = 0.01 * rng.standard_normal(N)

    def put(i, v):
        if 0 <= i < N:
            x[i] = v

    put(0, 0.9)
    put(N - 1, -0.8)
    put(TILE - 1, 0.7)
    put(TILE, -0.95)
    at = 40
    put(at, 0.85)
    put(at + 2 * H - 1, -0.6)
    at += 2 * H - 1 + 3 * H
    put(at, 0.75)
    put(at + 4 * H + 2, 0.65)
    at += 4 * H + 2 + 3 * H
    if at + 2 * H + 40 < N:
        x[at:at + 2 * H + 40] = 0.5
    at += 2 * H + 40 + 3 * H
    b = lr.quarter_rate_burst(min(512, max(N - at, 0)))
    if b.size >= 64:
        x[at:at + b.size] += 0.9 * b
    return x.astype(np.float32)


def cases():
    """(Q, us, N) of every shape the tests use"""
    return [(Q, us, N) for Q in GPU_RATES for us in LOOKAHEADS for N in lengths(Q, us)]


GAIN0, CEIL = 1.7, 0.7079457843841379   # the stage alone: a static gain that drives the features over a -3 dBTP ceiling
