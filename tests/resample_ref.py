"""fp64 restatement of the output-rate stage (include/xdtts.h, "The output rate"): the plan, the taps, the convolution from
a given tap array, and the a-priori error bound of an fp32 evaluation.  numpy only; the GPU tests compare against this."""
from math import gcd

import numpy as np

RATE_IN = 22050
RATES = (8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 88200, 96000)
RHO, BETA = 0.9, 10.0


def supported(Q):
    return 8000 <= Q <= 96000 and (Q == RATE_IN or Q // gcd(Q, RATE_IN) <= 640)


def plan(Q, n_in=0):
    """{"L", "M", "half_len", "n_out"}: L = Q / g, M = R / g, H = 32 max(L, M), N' = ceil(N L / M); the identity has no filter."""
    assert supported(Q), Q
    if Q == RATE_IN:
        return {"L": 1, "M": 1, "half_len": 0, "n_out": int(n_in)}
    g = gcd(Q, RATE_IN)
    L, M = Q // g, RATE_IN // g
    return {"L": L, "M": M, "half_len": 32 * max(L, M), "n_out": -((-int(n_in) * L) // M)}


def taps(Q):
    """h[k + H], k = -H .. H, in double."""
    p = plan(Q)
    L, M, H = p["L"], p["M"], p["half_len"]
    W = max(L, M)
    k = np.arange(-H, H + 1, dtype=np.float64)
    win = np.i0(BETA * np.sqrt(np.maximum(1.0 - (k / H) ** 2, 0.0))) / np.i0(BETA)
    return (L / W) * RHO * np.sinc(RHO * k / W) * win


def convolve(x, h, Q, m=None):
    """y[m] = sum over 0 <= n < N, |m M - n L| <= H of x[n] h[m M - n L] in fp64, from the tap array h (2 H + 1 values), for all
    m < N' or the given ones.  Returns (y, c, a): c[m] = the number of taps that meet output m, a[m] = sum |h| |x|."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    p = plan(Q, x.size)
    L, M, H = p["L"], p["M"], p["half_len"]
    assert h.size == 2 * H + 1
    m = np.arange(p["n_out"], dtype=np.int64) if m is None else np.asarray(m, dtype=np.int64)
    if m.size == 0:
        return np.zeros(0), np.zeros(0, np.int64), np.zeros(0)
    T = 2 * H // L + 2
    n = -((-(m * M - H)) // L)[:, None] + np.arange(T, dtype=np.int64)[None, :]  # from ceil((m M - H) / L) upward
    k = (m * M)[:, None] - n * L
    ok = (np.abs(k) <= H) & (n >= 0) & (n < x.size)
    xv = np.where(ok, x[np.clip(n, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
    hv = np.where(ok, h[np.clip(k + H, 0, 2 * H)], 0.0)
    return (xv * hv).sum(axis=1), ok.sum(axis=1), (np.abs(xv) * np.abs(hv)).sum(axis=1)


def bound(c, a):
    """|y_fp32 - y_fp64| per sample for any summation order of c fp32 products, fused or not: (c + 2) 2^-24 a."""
    return (np.asarray(c, dtype=np.float64) + 2.0) * 2.0 ** -24 * np.asarray(a, dtype=np.float64)
