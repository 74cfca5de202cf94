"""Single Pass Spectrogram Inversion as the vocoder's initial phase (phase_init mode 1; include/xdtts.h)
restated in numpy: the frame maps, the recurrence in its sequential and in its segment-scanned form, the angles, and a small
fp64 fast-Griffin-Lim with the handle's conventions for the property the stage exists for.

S crosses the boundary as (n_bins, F), C order, like every magnitude of the library; the definition itself is time-major.
Phases are uint32 in units of 2^-32 turn, every sum is modulo 2^32: the scan is exact in any order."""
import numpy as np

from prosody_ref import HOP, N_FFT, NB, stft_magnitude

U32 = np.uint32
HALF_TURN = np.uint32(1 << 31)


def frame_maps(S):
    """S (513, F) float32 -> (own (F, 513) int64, delta (F, 513) uint32): frame t maps phi_{t-1} to
    phi_t[j] = phi_{t-1}[own[t, j]] + delta[t, j]."""
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T)  # [F][513]
    F = St.shape[0]
    j = np.arange(NB)
    own = np.empty((F, NB), dtype=np.int64)
    delta = np.zeros((F, NB), dtype=U32)
    f32 = np.float32
    for t in range(F):
        m = St[t]
        peak = np.zeros(NB, dtype=bool)
        with np.errstate(invalid="ignore"):
            peak[1:-1] = (m[1:-1] > m[:-2]) & (m[1:-1] >= m[2:])
        if not peak.any():
            own[t] = j
            continue
        k = np.nonzero(peak)[0]
        a, b, c = m[k - 1], m[k], m[k + 1]
        with np.errstate(all="ignore"):
            d = (a - b) + (c - b)
            p = np.where(d == 0, f32(0), (f32(0.5) * (a - c)) / d).astype(f32)
            p = np.fmin(np.fmax(p, f32(-0.5)), f32(0.5))  # (fmaxf / fminf: a NaN becomes -0.5)
        assert p.dtype == f32
        frac = np.rint(p.astype(np.float64) * 2.0**30).astype(np.int64)  # exact: a power-of-two scale of an fp32
        adv = np.zeros(NB, dtype=np.int64)
        adv[k] = (((k & 3) << 30) + frac) & 0xFFFFFFFF
        pk = np.zeros(NB, dtype=f32)
        pk[k] = p
        left = np.maximum.accumulate(np.where(peak, j, -1))  # nearest peak at or below j, -1: none
        right = np.minimum.accumulate(np.where(peak, j, 1 << 20)[::-1])[::-1]  # nearest peak at or above j, 2^20: none
        has_l, has_r = left >= 0, right < (1 << 20)
        o = np.where(has_l & has_r, np.where(j - left <= right - j, left, right), np.where(has_l, left, right))
        pp = pk[o]
        flip = np.where(pp > 0, (j < o) | (j == o + 1), (j > o) | (j == o - 1)) & (j != o)
        own[t] = o
        delta[t] = ((adv[o] + np.where(flip, 1 << 31, 0)) & 0xFFFFFFFF).astype(U32)
    return own, delta


def sequential(own, delta):
    """turns (F, 513) uint32 by the recurrence, phi_{-1} = 0."""
    F = own.shape[0]
    out = np.empty((F, NB), dtype=U32)
    phi = np.zeros(NB, dtype=U32)
    for t in range(F):
        phi = phi[own[t]] + delta[t]  # (uint32 arithmetic wraps)
        out[t] = phi
    return out


def scanned(own, delta, L):
    """The same in the three steps the device takes: every segment of L frames composes its maps, one walk over the
    composites gives each segment's entry phase, every segment steps its frames from its entry."""
    F = own.shape[0]
    starts = list(range(0, F, L))
    comps = []
    for s in starts:
        O, D = np.arange(NB), np.zeros(NB, dtype=U32)
        for t in range(s, min(s + L, F)):
            O, D = O[own[t]], D[own[t]] + delta[t]
        comps.append((O, D))
    entries, carry = [], np.zeros(NB, dtype=U32)
    for O, D in comps:
        entries.append(carry)
        carry = carry[O] + D
    out = np.empty((F, NB), dtype=U32)
    for s, phi in zip(starts, entries):
        for t in range(s, min(s + L, F)):
            phi = phi[own[t]] + delta[t]
            out[t] = phi
    return out


def turns(S):
    """S (513, F) -> turns (513, F) uint32, the boundary layout of xdtts_griffinlim_spsi_phase."""
    return np.ascontiguousarray(sequential(*frame_maps(S)).T)


def angles(turns_):
    """turns (..) uint32 -> (.., 2) float64 (cos, sin) of u = float32(phi >> 8) * 2^-24 turns."""
    u = (np.asarray(turns_, dtype=U32) >> U32(8)).astype(np.float64) * 2.0**-24
    return np.stack([np.cos(2 * np.pi * u), np.sin(2 * np.pi * u)], axis=-1)


# ---- a small fp64 fast Griffin-Lim under the handle's conventions (1024 / 256, periodic Hann, centred, reflect padding) ----
_WIN = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)


def _istft(X):
    """X (513, F) complex -> HOP * (F - 1) samples (window-sum normalised, centre trimmed)."""
    F = X.shape[1]
    fr = np.fft.irfft(X.T, n=N_FFT, axis=1) * _WIN
    n = N_FFT + HOP * (F - 1)
    y, w = np.zeros(n), np.zeros(n)
    for t in range(F):
        y[t * HOP : t * HOP + N_FFT] += fr[t]
        w[t * HOP : t * HOP + N_FFT] += _WIN**2
    return (y / np.maximum(w, 1e-11))[N_FFT // 2 : N_FFT // 2 + HOP * (F - 1)]


def _stft(y):
    pad = np.pad(y, N_FFT // 2, mode="reflect")
    F = y.size // HOP + 1
    frames = np.stack([pad[j * HOP : j * HOP + N_FFT] * _WIN for j in range(F)])
    return np.fft.rfft(frames, axis=1).T


def griffinlim(S, ang0, iters, momentum=0.99):
    """Fast Griffin-Lim from the unit-modulus angles ang0 (513, F) complex: `iters` iterations, then the final ISTFT."""
    S = np.asarray(S, dtype=np.float64)
    ang, prev = np.asarray(ang0, dtype=np.complex128), np.zeros(S.shape, dtype=np.complex128)
    alpha = momentum / (1.0 + momentum)
    for _ in range(iters):
        reb = _stft(_istft(S * ang))
        ang = reb - alpha * prev
        prev = reb
        ang = ang / (np.abs(ang) + 1e-16)
    return _istft(S * ang)


def random_angles(F, seed):
    return np.exp(2j * np.pi * np.random.default_rng(seed).random((NB, F)))


def spsi_angles(S):
    a = angles(turns(np.asarray(S, dtype=np.float32)))
    return a[..., 0] + 1j * a[..., 1]


def spectral_convergence(y, S):
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(stft_magnitude(y) - S) / np.linalg.norm(S))
