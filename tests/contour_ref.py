"""Prosody contours (xdtts_prosody_contour, include/xdtts.h) restated in numpy: the value of a field at a position, the frame
table {c, pitch, gain}, F', and the stage itself.  contour(S, points, ..., dtype=np.float64) is the reference;
dtype=np.float32 is the same definition with every device operation in single precision (the table is host arithmetic in
double either way).  Both also say which branch -- copy (pitch exactly 1) or transform -- each output frame took.
The signal and measuring helpers are those of prosody_ref."""
import numpy as np
import scipy.fft

import prosody_ref as pr

N_FFT, NB = pr.N_FFT, pr.NB

# the five contours of the GPU parity test, (pos, rate, pitch, gain) each
CONTOURS = {
    "ramp": [(0.0, 1.0, 1.0, 1.0), (0.4, 1.0, 1.0, 1.0), (1.0, 1.6, 1.3, 0.5)],
    "step": [(0.0, 2.0, 0.8, 1.0), (0.5, 2.0, 0.8, 1.0), (0.5, 0.5, 1.25, 2.0)],
    "one": [(0.3, 0.7, 1.3, 1.0)],
    "mute": [(0.0, 1.0, 1.0, 1.0), (0.5, 1.0, 1.0, 0.0), (1.0, 4.0, 1.0, 0.0)],
    "five": [(0.1, 0.25, 2.0, 1.0), (0.2, 4.0, 0.5, 8.0), (0.2, 1.0, 1.0, 1.0), (0.6, 1.0, 1.0, 1.0), (0.9, 1.25, 0.9, 1.5)],
}
IDENTITY = [(0.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0)]


def _points(points):
    """The points as the C struct holds them (float32), widened to double: columns pos, rate, pitch, gain."""
    return np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 4)


def is_identity(points):
    return bool(np.all(_points(points)[:, 1:] == 1.0))


def field(pos, v, x):
    """v at the positions x (double): k = the number of points with pos <= x; v[0] before the first point, v[n-1] from the last
    on, else v[a] + (v[b] - v[a]) * ((x - pos[a]) / (pos[b] - pos[a])) with a = k - 1, b = k -- in this order of operations."""
    x = np.asarray(x, dtype=np.float64)
    n = len(pos)
    k = np.searchsorted(pos, x, side="right")
    a, b = np.clip(k - 1, 0, n - 1), np.clip(k, 0, n - 1)
    span = pos[b] - pos[a]
    safe = np.where(span > 0, span, 1.0)
    mid = v[a] + (v[b] - v[a]) * ((x - pos[a]) / safe)
    return np.where(k == 0, v[0], np.where(k == n, v[n - 1], mid))


def table(points, F):
    """(c uint32 [F], pitch float32 [F], gain float32 [F]) for F >= 2 input frames; C = c[F - 1] stays an exact integer."""
    P = _points(points)
    pos, rate, pitch, gain = P.T
    m = np.arange(F, dtype=np.float64)
    q = np.floor(65536.0 / field(pos, rate, (m[:-1] + 0.5) / (F - 1)) + 0.5).astype(np.uint64)
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(q, dtype=np.uint64)])
    assert int(c[-1]) < 2**32
    x = m / (F - 1)
    return c.astype(np.uint32), field(pos, pitch, x).astype(np.float32), field(pos, gain, x).astype(np.float32)


def frames_of(C):
    return max((int(C) + 32768) >> 16, 1) + 1


def frames(points, F):
    """F' behind the stage: F for the identity, else from the table."""
    if is_identity(points):
        return int(F)
    return frames_of(table(points, F)[0][-1])


def _pitch_frame(St, pitch, lifter, log_floor, t):
    """One frame through the pitch branch of xdtts_prosody, every operation in `t`: St [513] -> exp(E + R')."""
    L = np.log(np.maximum(St, log_floor))
    m = np.arange(N_FFT)
    ext = np.minimum(m, N_FFT - m)
    cep = (scipy.fft.fft(L[ext]).real / t(N_FFT)).astype(t)
    cep[(m > lifter) & (m < N_FFT - lifter)] = 0
    E = scipy.fft.fft(cep).real[:NB].astype(t)
    R = L - E
    p = np.arange(NB, dtype=t) / pitch
    inside = p <= NB - 1
    fl = np.floor(p)
    q = np.minimum(fl.astype(np.int64), NB - 1)
    a = np.where(inside, p - fl, t(0)).astype(t)
    Rw = np.where(inside, (t(1) - a) * R[q] + a * R[np.minimum(q + 1, NB - 1)], t(0))
    out = np.exp(E + Rw)
    assert out.dtype == t
    return out


def contour(S, points, lifter=30, log_floor=1e-5, dtype=np.float64):
    """S (513, F) -> (S' (513, F'), copied): copied[j] is True where output frame j took the copy branch (pitch exactly 1)."""
    t = dtype
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T).astype(t)  # [F][513]
    F = St.shape[0]
    if is_identity(points):
        return np.ascontiguousarray(St.T), np.ones(F, dtype=bool)
    c, pt, gn = table(points, F)
    C, Fp = int(c[-1]), frames_of(c[-1])
    floor_t = t(np.float32(log_floor))
    out = np.empty((Fp, NB), dtype=t)
    copied = np.zeros(Fp, dtype=bool)
    for j in range(Fp):
        tt = min(j * 65536, C)
        i = min(int(np.searchsorted(c, tt, side="right")) - 1, F - 2)
        num, den = tt - int(c[i]), int(c[i + 1]) - int(c[i])  # integers below 2^24: exact in float32
        w = t(np.float32(num)) / t(np.float32(den)) if t == np.float32 else t(num) / t(den)
        frame = (t(1) - w) * St[i] + w * St[i + 1]
        pj = t(pt[i]) + w * (t(pt[i + 1]) - t(pt[i]))
        gj = t(gn[i]) + w * (t(gn[i + 1]) - t(gn[i]))
        copied[j] = pj == 1
        out[j] = gj * frame if copied[j] else gj * _pitch_frame(frame, pj, lifter, floor_t, t)
    assert out.dtype == t
    return np.ascontiguousarray(out.T), copied
