"""fp64 restatement of the loudness stage (include/xdtts.h, "Loudness-normalised output"): the K-weighting coefficients, the
block plan, the gates, the true-peak filter, the gain rule, and the inputs the GPU tests use.  numpy and scipy.signal.lfilter;
the GPU tests compare against this."""
import numpy as np
from scipy.signal import lfilter

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000)   # the ten common rates
GPU_RATES = (8000, 11025, 22050, 48000, 96000)
OFFSET = -0.691
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
TP_BETA = 8.0
BS1770_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (-1.69065929318241, 0.73248077421585),
              (-1.99004745483398, 0.99007225036621))   # shelf b, shelf a1 a2, high-pass a1 a2


def supported(Q):
    return 8000 <= Q <= 96000


def coef(Q):
    """((b_shelf, a_shelf), (b_highpass, a_highpass)), a0 = 1, by the bilinear transform with K = tan(pi f0 / Q)."""
    f0, G, Qf = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / Q)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Qf + K * K
    shelf = (np.array([Vh + Vb * K / Qf + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Qf + K * K]) / a0,
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Qf + K * K) / a0]))
    f0, Qf = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / Q)
    a0 = 1.0 + K / Qf + K * K
    hp = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Qf + K * K) / a0]))
    return shelf, hp


def plan(Q, n=0):
    h = (Q + 5) // 10
    return {"hop": h, "n_blocks": (int(n) - 4 * h) // h + 1 if n >= 4 * h else 0}


def kweight(x, Q):
    (b1, a1), (b2, a2) = coef(Q)
    return lfilter(b2, a2, lfilter(b1, a1, np.asarray(x, dtype=np.float64)))


def kappa(Q, n=1 << 16):
    """The transient gain of the double pole: the largest factor by which an error in one state variable of the high-pass
    reaches a later output sample, max over n and i of |(c A^n)_i| -- A the state-transition matrix in the form the library runs
    (transposed direct form II), c = (1, 0) the row that reads the output.  For a double pole at r it is about 1 / (e (1 - r))."""
    a = coef(Q)[1][1]
    A = np.array([[-a[1], 1.0], [-a[2], 0.0]])
    row, worst = np.array([1.0, 0.0]), 1.0
    for _ in range(n):
        row = row @ A
        worst = max(worst, float(np.abs(row).max()))
    return worst


def true_peak_taps():
    """t[p - 1][j + 12] = t[4 j + p] in double: sinc(k / 4) I0(8 sqrt(1 - (k / 48)^2)) / I0(8)."""
    p = np.arange(1, 4)[:, None]
    j = np.arange(-12, 12)[None, :]
    k = (4 * j + p).astype(np.float64)
    return np.sinc(k / 4.0) * np.i0(TP_BETA * np.sqrt(1.0 - (k / 48.0) ** 2)) / np.i0(TP_BETA)


def true_peak(x, taps=None):
    """(true peak, sample peak, bound): the largest magnitude over x and y[4 n + p] = sum_j x[n - j] t[4 j + p], n = 0 .. N - 1,
    from the given tap array (default: the double taps); bound = the largest a-priori error of an fp32 evaluation of one phase
    value, (24 + 2) 2^-24 sum |t| |x| (resample_ref.bound)."""
    from resample_ref import bound

    x = np.asarray(x, dtype=np.float64)
    t = true_peak_taps() if taps is None else np.asarray(taps, dtype=np.float64)
    xp = np.concatenate([np.zeros(12), x, np.zeros(12)])
    # x[n - j] for j = -12 .. 11 is xp[n + 12 - j]: a window of 24 from xp[n + 1], reversed
    win = np.lib.stride_tricks.sliding_window_view(xp, 24)[1:x.size + 1, ::-1]
    y = win @ t.T
    a = np.abs(win) @ np.abs(t).T
    sp = float(np.max(np.abs(x))) if x.size else 0.0
    tp = max(sp, float(np.max(np.abs(y)))) if x.size else 0.0
    return tp, sp, float(np.max(bound(24, a))) if x.size else 0.0


def measure(x, Q):
    """The whole measurement in fp64: dict with z (block means), abs_mask, mask (both gates), rel_gate, mean_square,
    blocks, gated_blocks, lufs, true_peak, sample_peak."""
    x = np.asarray(x, dtype=np.float64)
    p = plan(Q, x.size)
    h, nb = p["hop"], p["n_blocks"]
    y2 = kweight(x, Q) ** 2
    z = np.array([y2[j * h: j * h + 4 * h].mean() for j in range(nb)], dtype=np.float64)
    abs_mask = z > ABS_GATE
    rel = 0.1 * z[abs_mask].mean() if abs_mask.any() else np.inf
    mask = abs_mask & (z > rel)
    Z = float(z[mask].mean()) if mask.any() else 0.0
    tp, sp, _ = true_peak(x)
    return {"z": z, "abs_mask": abs_mask, "mask": mask, "rel_gate": rel, "mean_square": Z, "blocks": nb,
            "gated_blocks": int(mask.sum()), "lufs": lufs(Z), "true_peak": tp, "sample_peak": sp}


def lufs(Z):
    return OFFSET + 10.0 * np.log10(Z) if Z > 0 else -np.inf


def gain(Z, tp, target, ceiling=None):
    if not Z > 0:
        return 1.0
    g = 10.0 ** ((target + 0.691) / 20.0) / np.sqrt(Z)
    if ceiling is not None and not np.isnan(ceiling) and g * tp > 10.0 ** (ceiling / 20.0):
        g = 10.0 ** (ceiling / 20.0) / tp
    return g


def gate_margin(m):
    """The smallest relative distance of a block mean from either gate threshold (inf without blocks)."""
    z = m["z"]
    if z.size == 0:
        return np.inf
    d = np.abs(z - ABS_GATE) / ABS_GATE
    if np.isfinite(m["rel_gate"]):
        d = np.minimum(d, np.abs(z - m["rel_gate"]) / m["rel_gate"])
    return float(d.min())


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------

def lengths(Q):
    """No block, exactly one block, a segment that straddles a sub-block boundary, more than 64 segments, more than one group."""
    h = plan(Q)["hop"]
    return (1, 4 * h - 1, 4 * h, 5 * h - 1, 5 * h + 1, 25 * h + 13)


def ragged_lengths(Q):
    h = plan(Q)["hop"]
    return (1, 25 * h + 13, 4 * h - 1, 5 * h, 4 * h)


def speech_like(Q, N, seed=0):
    """fp32, N samples at rate Q: a loud modulated tone plus noise; from 40 % to 60 % of the length a stretch 40 dB lower (only
    the relative gate removes it); from 60 % to 80 % digital silence (the absolute gate removes it); then loud again."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    t = np.arange(N) / float(Q)
    x = 0.25 * np.sin(2 * np.pi * 220.0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.1 * t)) + 0.02 * rng.standard_normal(N)
    pos = np.arange(N) / max(N, 1)
    x = np.where((pos >= 0.4) & (pos < 0.6), 0.01 * x, x)
    x = np.where((pos >= 0.6) & (pos < 0.8), 0.0, x)
    return x.astype(np.float32)


def sine(Q, f=997.0, seconds=3.0, amp=1.0):
    return amp * np.sin(2 * np.pi * f * np.arange(int(round(seconds * Q))) / Q)


def quarter_rate_burst(n=512):
    """fs/4 sine at 45 degrees under a Hann taper: every sample of the carrier sits at +-sin(45 deg), 3.01 dB under the peak
    of the waveform between the samples."""
    k = np.arange(n)
    return np.sin(np.pi / 2.0 * k + np.pi / 4.0) * np.hanning(n)
