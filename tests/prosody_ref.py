"""The prosody stage (xdtts_prosody, include/xdtts.h) restated in numpy, and the signal and the measuring helpers its tests use.

prosody(S, ..., dtype=np.float64) is the reference; dtype=np.float32 is the same definition with every operation in single
precision (scipy.fft stays in float32 where numpy.fft would go through double) -- the yardstick of what fp32 arithmetic costs.
S crosses the boundary as (n_bins, F), C order, like every magnitude of the library; the definition itself is time-major."""
import numpy as np
import scipy.fft

N_FFT, HOP, NB, SR = 1024, 256, 513, 22050


def prosody_frames(F, rate):
    """F' = F at rate 1, else max(floor((F - 1) / rate + 0.5), 1) + 1 -- in double, from the float32 rate the library receives."""
    rate = float(np.float32(rate))
    if rate == 1.0:
        return int(F)
    return int(max(np.floor((F - 1) / rate + 0.5), 1.0)) + 1


def prosody(S, rate=1.0, pitch=1.0, lifter=30, log_floor=1e-5, dtype=np.float64):
    """S (513, F) -> S' (513, F').  The parameters are rounded to float32 first (what the C struct holds); u_j = j * rate and
    p = k / pitch are then evaluated in `dtype` -- the fp32 kernel's own rounding of them is part of what the yardstick shows."""
    t = dtype
    rate, pitch, log_floor = (t(np.float32(x)) for x in (rate, pitch, log_floor))
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T).astype(t)  # [F][513]
    F = St.shape[0]
    if rate != 1:
        Fp = prosody_frames(F, rate)
        u = np.minimum(np.arange(Fp, dtype=t) * rate, t(F - 1))
        i = np.minimum(np.floor(u).astype(np.int64), F - 2)
        w = (u - i.astype(t))[:, None]
        St = (t(1) - w) * St[i] + w * St[i + 1]
    assert St.dtype == t
    if pitch == 1:
        return np.ascontiguousarray(St.T)
    L = np.log(np.maximum(St, log_floor))
    m = np.arange(N_FFT)
    ext = np.minimum(m, N_FFT - m)
    c = (scipy.fft.fft(L[:, ext], axis=1).real / t(N_FFT)).astype(t)  # the real cepstrum: inverse DFT of a real even sequence
    c[:, (m > lifter) & (m < N_FFT - lifter)] = 0
    E = scipy.fft.fft(c, axis=1).real[:, :NB].astype(t)
    R = L - E
    p = np.arange(NB, dtype=t) / pitch
    inside = p <= NB - 1
    q = np.minimum(np.floor(p).astype(np.int64), NB - 1)
    a = np.where(inside, p - np.floor(p), t(0)).astype(t)
    Rw = (t(1) - a) * R[:, q] + a * R[:, np.minimum(q + 1, NB - 1)]
    Rw = np.where(inside[None, :], Rw, t(0))
    out = np.exp(E + Rw)
    assert out.dtype == t
    return np.ascontiguousarray(out.T)


def rel_err(x, ref64, log_floor=1e-5):
    """max |x - ref64| / max(ref64, log_floor) over all cells."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.max(np.abs(x - ref64) / np.maximum(ref64, log_floor)))


def random_magnitude(F, seed=0):
    """(513, F) float32: log-uniform over nine e-folds (e^-9 .. 1), 5 % of the cells exactly zero."""
    rng = np.random.default_rng(seed)
    S = np.exp(rng.uniform(-9.0, 0.0, size=(NB, F)))
    S[rng.random((NB, F)) < 0.05] = 0.0
    return S.astype(np.float32)


def voiced_signal(n=HOP * 47, f0=140.0, vibrato=0.03, seed=0):
    """A synthetic voiced sound: a harmonic series on f0 with a 5 Hz vibrato of +-3 %, shaped by three formants (700, 1220,
    2600 Hz), a little noise.  float32, peak 0.5."""
    t = np.arange(n) / SR
    phase = 2 * np.pi * f0 * (t - vibrato / (2 * np.pi * 5.0) * np.cos(2 * np.pi * 5.0 * t))  # d/dt = 2 pi f0 (1 + v sin(2 pi 5 t))
    y = np.zeros(n)
    for h in range(1, int(0.45 * SR / (f0 * (1 + vibrato)))):
        f = h * f0
        gain = sum(g / (1.0 + ((f - fc) / bw) ** 2) for fc, bw, g in ((700.0, 130.0, 1.0), (1220.0, 170.0, 0.5), (2600.0, 250.0, 0.25)))
        y += (gain + 0.003) * np.sin(h * phase)
    y += 1e-3 * np.random.default_rng(seed).standard_normal(n)
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


def stft_magnitude(y):
    """|librosa.stft(y, 1024, hop 256, periodic hann, center, reflect)| in fp64: (513, len(y) // 256 + 1)."""
    y = np.asarray(y, dtype=np.float64)
    pad = np.pad(y, N_FFT // 2, mode="reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    F = y.size // HOP + 1
    frames = np.stack([pad[j * HOP : j * HOP + N_FFT] * win for j in range(F)])
    return np.abs(np.fft.rfft(frames, axis=1)).T


def cepstral_peak(S, lo=60, hi=400, log_floor=1e-5):
    """Per frame, the quefrency (samples at 22050 Hz) of the largest real-cepstrum value in [lo, hi]: the pitch period.
    S is (513, F); returns F integers."""
    L = np.log(np.maximum(np.asarray(S, dtype=np.float64).T, log_floor))
    c = np.fft.irfft(L, n=N_FFT, axis=1)
    return lo + np.argmax(c[:, lo : hi + 1], axis=1)


def _frame_f0(seg, lo, hi):
    """F0 of one analysis window: the first local maximum of its normalised autocorrelation in lags [lo, hi] that comes within
    10 % of the largest one there (the first, so that a multiple of the period is not taken for it), refined by a parabola
    through its neighbours.  The window is a Hann; its own autocorrelation is divided out."""
    n = seg.size
    w = np.hanning(n)

    def autocorr(x):
        spec = np.fft.rfft(x, 2 * n)
        return np.fft.irfft(spec * np.conj(spec))[:n]

    ac = autocorr((seg - seg.mean()) * w) / np.maximum(autocorr(w), 1e-9)
    ac = ac / ac[0]
    top = ac[lo : hi + 1].max()
    k = next(k for k in range(lo, hi + 1) if ac[k] >= 0.9 * top and ac[k] >= ac[k - 1] and ac[k] >= ac[k + 1])
    a, b, c = ac[k - 1], ac[k], ac[k + 1]
    d = 0.5 * (a - c) / (a - 2 * b + c) if (a - 2 * b + c) != 0 else 0.0
    return SR / (k + d)


def f0_autocorr(y, lo_hz=60.0, hi_hz=400.0, win=2048, hop=HOP):
    """F0 (Hz) of a stretch of audio: the median over windows of `win` samples (93 ms: five periods at the low end) of the
    short-time autocorrelation estimate.  Short windows because the signal has vibrato: over a long one the period's peak
    smears out while the peaks of the (fixed) formants do not."""
    y = np.asarray(y, dtype=np.float64)
    lo, hi = int(SR / hi_hz), int(SR / lo_hz)
    return float(np.median([_frame_f0(y[s : s + win], lo, hi) for s in range(0, y.size - win + 1, hop)]))
