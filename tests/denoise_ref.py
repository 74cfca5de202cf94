"""The clean-up stage's definition (include/xdtts.h, the xdtts_denoise block) restated in numpy, operation by operation in fp32:
the yardstick of xdtts_denoise_reference (bit for bit) and, through it, of the device.  gmin and E come from the library's host
functions (xdtts_denoise_floor / _tone), so that the single libm call decides no bit here; test_denoise_cpu.py holds those two to
1 ulp of numpy's 10 ** (x / 20) separately.  Also the crafted inputs the CPU and GPU tests share."""
import numpy as np

NB = 513
F32 = np.float32


def rank(F, quantile):
    return int(np.floor(float(F32(quantile)) * (F - 1)))


def keys(S):
    return np.ascontiguousarray(S, dtype=F32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def noise(S, quantile):
    """N[k]: the float whose bits are the r-th smallest key over the frames of S (513, F)."""
    k = np.sort(keys(S), axis=1)
    return np.ascontiguousarray(k[:, rank(S.shape[1], quantile)]).view(F32)


def tone_is_flat(d):
    return all(d.tone_db[i] == 0.0 for i in range(d.n_tone))


def denoise(S, d, gmin, E, profile=None):
    """S (513, F) fp32 -> (S', (cells, floored, rank, profiled)); every operation a single fp32 numpy operation."""
    S = np.ascontiguousarray(S, dtype=F32)
    F = S.shape[1]
    sub = d.strength != 0.0
    out = S.copy()
    floored, r, profiled = 0, 0, 0
    if sub:
        if profile is None:
            r = rank(F, d.quantile)
            N = noise(S, d.quantile)
        else:
            N, profiled = np.asarray(profile, dtype=F32), 1
        aN = (F32(d.strength) * N).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = (aN[:, None] / S).astype(F32)
            dd = (F32(1.0) - q).astype(F32)
            above = dd > F32(gmin)  # (False for a NaN)
            G = np.where(above, dd, F32(gmin)).astype(F32)
            out = (S * G).astype(F32)
        floored = int(np.count_nonzero(~above))
    if not tone_is_flat(d):
        with np.errstate(over="ignore", invalid="ignore"):
            out = (out * np.asarray(E, dtype=F32)[:, None]).astype(F32)
    return out, (NB * F, floored, r, profiled)


# ---- the crafted input: 513 bins of which the first columns are the hard cases, the rest log-uniform over nine e-folds ----

def crafted(F, seed=0):
    """(513, F) fp32, no subnormals, no negatives: bin 0 a constant, bin 1 four distinct values, bin 2 more than r + 1 exact zeros
    for every r < F (all but one zero; N = 0, q = 0 / 0 where S = 0), bin 3 consecutive floats (only the last radix pass decides),
    bin 4 values that differ in the top byte only, bin 512 (the lone strip) consecutive floats in reverse; everything else
    log-uniform over nine e-folds with 2 % exact zeros."""
    rng = np.random.default_rng(1000 + 7 * F + seed)
    S = np.exp(rng.uniform(-9.0, 0.0, size=(NB, F))).astype(F32)
    S[rng.random((NB, F)) < 0.02] = 0.0
    S[0] = F32(0.125)
    S[1] = np.array([0.5, 0.25, 1.5, 3.0], dtype=F32)[rng.integers(0, 4, F)]
    S[2] = 0.0
    S[2, rng.integers(0, F)] = 0.75
    chain = np.empty(F, dtype=F32)
    x = F32(0.3)
    for i in range(F):
        chain[i] = x
        x = np.nextafter(x, F32(1.0))
    S[3] = chain[rng.permutation(F)]
    top = (np.uint32(0x10) + (rng.permutation(F).astype(np.uint32) % np.uint32(0x60))) << np.uint32(24) | np.uint32(0x00345678)
    S[4] = top.view(F32)  # exponent bytes 0x10 .. 0x6f: normal, finite
    S[512] = chain[::-1]
    assert np.all(np.isfinite(S)) and np.all(S >= 0)
    assert not np.any((S != 0) & (np.abs(S) < np.finfo(F32).tiny))
    return S


def tone_scene(F, seed=0, zeros=True):
    """Rayleigh noise of scale 1e-3 in every cell and a three-harmonic tone of magnitude 1 wandering over the middle 60 % of the
    frames; 2 % exact zeros sprinkled into the noise-only cells.  -> (S (513, F), mask of the tone's cells)."""
    rng = np.random.default_rng(77 + F + seed)
    S = rng.rayleigh(1e-3, size=(NB, F)).astype(F32)
    tone = np.zeros((NB, F), dtype=bool)
    t0, t1 = int(round(0.2 * F)), int(round(0.8 * F))
    for t in range(t0, t1):
        b = 40 + int(round(6 * np.sin(2 * np.pi * (t - t0) / max(t1 - t0, 1))))
        for h in (1, 2, 3):
            tone[h * b, t] = True
    if zeros:
        S[(rng.random((NB, F)) < 0.02) & ~tone] = 0.0
    S[tone] = 1.0
    return S, tone
