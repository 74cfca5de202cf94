"""The timbre stage (xdtts_timbre, include/xdtts.h) restated in numpy, and the signals and measuring helpers its tests use.

timbre(S, ..., dtype=np.float64) is the reference; dtype=np.float32 is the same definition with every operation in single
precision (scipy.fft stays in float32 where numpy.fft would go through double) -- the yardstick of what fp32 arithmetic costs,
exactly as tests/prosody_ref.py does for the prosody stage.  S crosses the boundary as (n_bins, F), C order, like every
magnitude of the library; the definition itself is time-major."""
import numpy as np
import scipy.fft

import prosody_ref as pr

N_FFT, NB = pr.N_FFT, pr.NB
NOISE_STREAM = 0x71B8
NOISE_SHIFT = np.float32(0.28860784)  # gamma / 2 as the library's fp32 constant
GAMMA = 0.5772156649015329
# the analytic range of N: v = (2 n + 1) 2^-24 runs from 2^-24 to 1 - 2^-24, where -ln v = 24 ln 2 and (to first order) 2^-24
N_MIN = 0.5 * np.log(2.0 ** -24) + GAMMA / 2
N_MAX = 0.5 * np.log(24.0 * np.log(2.0)) + GAMMA / 2

# the parameter sets of the device == reference check: (vtl, breath)
CASES = ((1.25, 0.0), (0.7, 0.4), (1.0, 1.0), (2.0, 0.0), (0.5, 1.0))
VTL_FACTORS = (0.5, 0.8, 1.0 / 1.1, 1.25, 1.6, 2.0)


def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x = (x * np.uint32(0x7FEB352D)).astype(np.uint32)
    x ^= x >> np.uint32(15)
    x = (x * np.uint32(0x846CA68B)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    return x


def rng_u32(seed, stream, idx):
    """csrc/rng.h: mix32(mix32(mix32(seed ^ 0x9E3779B9) + stream) + idx), all modulo 2^32; idx an array."""
    with np.errstate(over="ignore"):
        a = _mix32(np.array([(int(seed) ^ 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint32))
        b = _mix32((a + np.uint32(stream)).astype(np.uint32))
        return _mix32((b + np.asarray(idx, dtype=np.uint32)).astype(np.uint32))


def noise_bits(seed, frame, bin_):
    """n of the cells (frame, bin): 23 bits; frame and bin broadcast."""
    with np.errstate(over="ignore"):
        idx = (np.asarray(frame, dtype=np.uint32) * np.uint32(NB) + np.asarray(bin_, dtype=np.uint32)).astype(np.uint32)
    return rng_u32(seed, NOISE_STREAM, idx) >> np.uint32(9)


def noise(seed, F, dtype=np.float64):
    """N [F][513]: 0.5 ln(-ln v) + gamma / 2 with v = (2 n + 1) 2^-24 (exact in either precision)."""
    t = dtype
    n = noise_bits(seed, np.arange(F)[:, None], np.arange(NB)[None, :])
    v = (2 * n.astype(np.int64) + 1).astype(t) * t(2.0 ** -24)
    out = t(0.5) * np.log(-np.log(v)) + t(NOISE_SHIFT)
    assert out.dtype == t
    return out


def timbre(S, vtl=1.0, breath=0.0, seed=1, lifter=30, log_floor=1e-5, dtype=np.float64, arithmetic=False):
    """S (513, F) -> S' (513, F).  The parameters are rounded to float32 first (what the C struct holds); p = k * vtl is then
    evaluated in `dtype`.  The identity returns S unless `arithmetic` asks for the path every other setting takes."""
    t = dtype
    vtl, breath, log_floor = (t(np.float32(x)) for x in (vtl, breath, log_floor))
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T).astype(t)  # [F][513]
    F = St.shape[0]
    if vtl == 1 and breath == 0 and not arithmetic:
        return np.ascontiguousarray(St.T)
    L = np.log(np.maximum(St, log_floor))
    m = np.arange(N_FFT)
    ext = np.minimum(m, N_FFT - m)
    c = (scipy.fft.fft(L[:, ext], axis=1).real / t(N_FFT)).astype(t)  # the real cepstrum: inverse DFT of a real even sequence
    c[:, (m > lifter) & (m < N_FFT - lifter)] = 0
    E = scipy.fft.fft(c, axis=1).real[:, :NB].astype(t)
    R = L - E
    p = np.arange(NB, dtype=t) * vtl
    inside = p <= NB - 1
    q = np.minimum(np.floor(p).astype(np.int64), NB - 1)
    a = np.where(inside, p - np.floor(p), t(0)).astype(t)
    Ew = (t(1) - a) * E[:, q] + a * E[:, np.minimum(q + 1, NB - 1)]
    Ew = np.where(inside[None, :], Ew, E[:, NB - 1 : NB])
    if breath != 0:
        R = (t(1) - breath) * R + breath * noise(seed, F, t)
    out = np.exp(Ew + R)
    assert out.dtype == t
    return np.ascontiguousarray(out.T)


rel_err = pr.rel_err
random_magnitude = pr.random_magnitude


# ---- the signals and measures of the three properties -----------------------------------------------------------------------

def voiced_magnitude():
    """|STFT| of prosody_ref.voiced_signal in fp64, as float32: (513, 48).  Its pitch period is 157 samples."""
    return pr.stft_magnitude(pr.voiced_signal()).astype(np.float32)


def cepstral_peak_value(S, lo=60, hi=400, log_floor=1e-5):
    """The median over frames of the largest real-cepstrum value at quefrencies lo .. hi: how much of a harmonic series the
    magnitude holds."""
    L = np.log(np.maximum(np.asarray(S, dtype=np.float64).T, log_floor))
    c = np.fft.irfft(L, n=N_FFT, axis=1)
    return float(np.median(c[:, lo : hi + 1].max(axis=1)))


def period(S):
    """The median pitch period (samples) over frames: prosody_ref.cepstral_peak."""
    return int(np.median(pr.cepstral_peak(S)))


def bump_magnitude(centre, F=3, sigma=20.0, floor=1e-3, period_samples=157.0, depth=0.8):
    """A Gaussian envelope bump on a floor, times a harmonic comb whose log is one cosine at the quefrency of the pitch period
    (far above the lifter, so the split puts the bump into E and the comb into R): (513, F) float32, all frames alike."""
    k = np.arange(NB, dtype=np.float64)
    env = floor + np.exp(-0.5 * ((k - centre) / sigma) ** 2)
    comb = np.exp(depth * np.cos(2 * np.pi * k * period_samples / N_FFT))
    return np.repeat((env * comb)[:, None], F, axis=1).astype(np.float32)


def power_centroid(S):
    """sum k S^2 / sum S^2 per frame, the median over frames."""
    P = np.asarray(S, dtype=np.float64) ** 2
    k = np.arange(NB, dtype=np.float64)[:, None]
    return float(np.median((k * P).sum(axis=0) / P.sum(axis=0)))


def check_properties(stage, say=None):
    """The three properties of the stage, asserted on stage(S, vtl=, breath=) -> S' -- the reference itself (the CPU test) or the
    device's hook (the GPU test): the same inputs, the same bounds.  Returns the figures."""
    fig = {}
    V = voiced_magnitude()
    base = cepstral_peak_value(V)
    assert period(V) == 157
    for vtl in (0.8, 1.25, 1.5):  # the formants move, the pitch stays
        out = stage(V, vtl=vtl, breath=0.0)
        fig["period vtl %g" % vtl] = period(out)
        fig["peak vtl %g" % vtl] = cepstral_peak_value(out)
    for breath in (0.5, 1.0):  # the harmonics give way to noise
        fig["peak ratio breath %g" % breath] = cepstral_peak_value(stage(V, vtl=1.0, breath=breath)) / base
    for centre in (120, 200):  # a formant at bin b moves to b / vtl
        B = bump_magnitude(centre)
        for vtl in VTL_FACTORS:
            fig["centroid %d vtl %.4g" % (centre, vtl)] = power_centroid(stage(B, vtl=vtl, breath=0.0)) - centre / float(np.float32(vtl))
    if say:
        say("cepstral peak of the voiced signal %.4f" % base)
        for key, v in fig.items():
            say("%s: %s" % (key, ("%d" % v) if key.startswith("period") else ("%+.4f" % v)))
    for vtl in (0.8, 1.25, 1.5):
        assert fig["period vtl %g" % vtl] == 157, (vtl, fig)
    assert fig["peak ratio breath 1"] <= 0.25, fig
    assert 0.4 <= fig["peak ratio breath 0.5"] <= 0.65, fig
    for key, v in fig.items():
        if key.startswith("centroid"):
            assert abs(v) <= 0.5, (key, v)
    return fig
