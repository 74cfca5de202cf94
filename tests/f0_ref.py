"""The pitch tracker and pitch targets (xdtts_f0_opts, xdtts_pitch_target; include/xdtts.h) restated in numpy.

dtype=np.float64 is the reference; dtype=np.float32 is the same definition with every device operation in single precision
(scipy.fft stays in float32) -- the yardstick of what fp32 arithmetic costs, the idiom of prosody_ref.  The utterance stage
compares and selects, so it is the same in both; its one piece of arithmetic, the ratio, takes log2 and exp2 correctly rounded
in float32 (through double, rounded once), as the definition says.  S crosses as (n_bins, F), like every magnitude of the library.
The signal and measuring helpers are those of prosody_ref; the pitch branch is contour_ref._pitch_frame."""
import math

import numpy as np
import scipy.fft

import contour_ref as cr
import prosody_ref as pr

N_FFT, NB, SR, HOP = pr.N_FFT, pr.NB, pr.SR, pr.HOP
DEFAULT_OPTS = dict(fmin=60.0, fmax=400.0, threshold=0.2, octave_bias=0.9, log_floor=1e-5)
F0_MAX_FRAMES = 16384


def opts(**kw):
    o = dict(DEFAULT_OPTS)
    o.update(kw)
    return o


def plan(fmin=60.0, fmax=400.0):
    """(q_lo, q_hi) = (ceil(22050 / fmax), floor(22050 / fmin)) in double, from the float32 fields the struct holds."""
    return int(math.ceil(22050.0 / float(np.float32(fmax)))), int(math.floor(22050.0 / float(np.float32(fmin))))


def opts_ok(o):
    f = [float(np.float32(o[k])) for k in ("fmin", "fmax", "threshold", "octave_bias", "log_floor")]
    if not all(math.isfinite(x) for x in f):
        return False
    fmin, fmax, thr, bias, floor = f
    if not (50.0 <= fmin < fmax <= 1000.0 and thr >= 0.0 and 0.0 < bias <= 1.0 and floor > 0.0):
        return False
    lo, hi = plan(fmin, fmax)
    return lo < hi


def target_ok(mode, value, rng):
    value, rng = float(np.float32(value)), float(np.float32(rng))
    if mode not in (0, 1, 2) or not math.isfinite(rng) or not 0.0 <= rng <= 4.0:
        return False
    if mode == 1 and not (math.isfinite(value) and 50.0 <= value <= 1000.0):
        return False
    if mode == 2 and not (math.isfinite(value) and 0.5 <= value <= 2.0):
        return False
    return True


def cepstrum(S, log_floor=1e-5, dtype=np.float64):
    """S (513, F) -> c [F][1024], the real cepstrum of ln max(S, log_floor) as xdtts_prosody forms it (a NaN cell becomes the floor)."""
    t = dtype
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T).astype(t)
    L = np.log(np.fmax(St, t(np.float32(log_floor))))
    m = np.arange(N_FFT)
    ext = np.minimum(m, N_FFT - m)
    c = (scipy.fft.fft(L[:, ext], axis=1).real / t(N_FFT)).astype(t)
    assert c.dtype == t
    return c


def pick(c, q_lo, q_hi, bias, margin=0.0):
    """n* of one frame's cepstrum c.  margin != 0 tightens (> 0) or loosens (< 0) every >= of the rule by that much: two runs
    with +-margin that agree say that no comparison of the rule lies within the margin of its threshold."""
    t = c.dtype.type
    seg = c[q_lo : q_hi + 1]
    valid = ~np.isnan(seg)
    if not valid.any():
        return q_lo
    top = seg[valid].max()
    if top > 0:
        thr = t(bias) * top
        n = np.arange(q_lo, q_hi + 1)
        with np.errstate(invalid="ignore"):
            ok = (seg >= thr + t(margin)) & (seg >= c[n - 1] + t(margin)) & (seg >= c[n + 1] + t(margin))
        if ok.any():
            return int(n[np.argmax(ok)])
    with np.errstate(invalid="ignore"):
        return q_lo + int(np.argmax(seg == top))


def offset(a, b, c, t):
    """SPSI's parabolic offset (include/xdtts.h, "offset") in `t`."""
    d = (a - b) + (c - b)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = t(0) if d == 0 else t(0.5) * (a - c) / d
    if np.isnan(p):  # fminf(fmaxf(NaN, -0.5), 0.5)
        p = t(-0.5)
    return min(max(p, t(-0.5)), t(0.5))


def frames(S, o=None, dtype=np.float64):
    """The per-frame stage: (n* int [F], raw [F], strength [F], c [F][1024]) in `dtype`."""
    o = opts() if o is None else o
    t = dtype
    q_lo, q_hi = plan(o["fmin"], o["fmax"])
    c = cepstrum(S, o["log_floor"], t)
    F = c.shape[0]
    ns = np.zeros(F, dtype=np.int64)
    raw, strength = np.zeros(F, dtype=t), np.zeros(F, dtype=t)
    bias = t(np.float32(o["octave_bias"]))
    for f in range(F):
        n = pick(c[f], q_lo, q_hi, bias)
        p = offset(c[f, n - 1], c[f, n], c[f, n + 1], t)
        ns[f] = n
        raw[f] = t(22050.0) / (t(n) + p)
        strength[f] = c[f, n]
    return ns, raw, strength, c


def ambiguous(c64, o, bound):
    """Frames of the fp64 cepstrum where some comparison of the n* rule lies within `bound` of its threshold (so that an fp32
    cepstrum within bound / 2 of it may decide otherwise): bool [F]."""
    q_lo, q_hi = plan(o["fmin"], o["fmax"])
    bias = np.float64(np.float32(o["octave_bias"]))
    out = np.zeros(c64.shape[0], dtype=bool)
    for f in range(c64.shape[0]):
        top = np.nanmax(c64[f, q_lo : q_hi + 1])
        near_zero = abs(top) <= bound
        out[f] = near_zero or pick(c64[f], q_lo, q_hi, bias, bound) != pick(c64[f], q_lo, q_hi, bias, -bound)
    return out


def _log2_32(x):
    return np.float32(np.log2(np.float64(x)))


def _exp2_32(x):
    return np.float32(np.exp2(np.float64(x)))


def track(raw, strength, o=None, target=(0, 1.0, 1.0), dtype=np.float32):
    """The utterance stage: (f0 float32 [F], voiced bool [F], ratio `dtype` [F], stats dict).  raw / strength are the float32
    arrays the device holds; the selections are exact, the ratio is evaluated in `dtype`."""
    o = opts() if o is None else o
    raw = np.asarray(raw, dtype=np.float32)
    strength = np.asarray(strength, dtype=np.float32)
    F = raw.size
    with np.errstate(invalid="ignore"):
        voiced = strength >= np.float32(o["threshold"])
    f0 = np.zeros(F, dtype=np.float32)
    for i in range(F):
        if not voiced[i]:
            continue
        a, b = max(i - 2, 0), min(i + 2, F - 1)
        w = np.sort(raw[a : b + 1][voiced[a : b + 1]])
        f0[i] = w[(w.size - 1) // 2]
    v = np.sort(f0[voiced])
    n_voiced = int(v.size)
    median = v[(n_voiced - 1) // 2] if n_voiced else np.float32(0)
    mode, value, rng = target
    value, rng = np.float32(value), np.float32(rng)
    t = dtype
    if t == np.float32:
        log2, exp2 = _log2_32, _exp2_32
    else:
        log2, exp2 = np.log2, np.exp2
    base = t(1)
    if n_voiced:
        base = t(value) / t(median) if mode == 1 else (t(value) if mode == 2 else t(1))
    lb = log2(base)
    ratio = np.full(F, base, dtype=t)
    if n_voiced:
        lm, rm1 = log2(t(median)), t(rng) - t(1)
        for i in range(F):
            if voiced[i]:
                d = log2(t(f0[i])) - lm
                pr_ = rm1 * d
                ratio[i] = exp2(lb + pr_)
    clamped = np.minimum(np.maximum(ratio, t(0.5)), t(2.0))
    stats = dict(n_frames=F, n_voiced=n_voiced, n_clamped=int(np.count_nonzero(clamped != ratio)), median_hz=np.float32(median),
                 min_hz=np.float32(v[0]) if n_voiced else np.float32(0), max_hz=np.float32(v[-1]) if n_voiced else np.float32(0),
                 base_ratio=np.float32(base) if t == np.float32 else base)
    assert clamped.dtype == t
    return f0, voiced, clamped, stats


def rate1_table(F):
    """The table of an utterance under a target without a contour: c[m] = 65536 m, pitch 1, gain 1."""
    return (np.arange(F, dtype=np.uint64) * 65536).astype(np.uint32), np.ones(F, dtype=np.float32), np.ones(F, dtype=np.float32)


def table_pitch(pitch, ratio):
    """pitch_m = clamp(fl(contour pitch_m * ratio[m])) in float32: what the device writes into the table."""
    p = np.asarray(pitch, dtype=np.float32) * np.asarray(ratio, dtype=np.float32)
    return np.minimum(np.maximum(p, np.float32(0.5)), np.float32(2.0)).astype(np.float32)


def apply_table(S, c, pitch, gain, lifter=30, log_floor=1e-5, dtype=np.float64):
    """The contour stage (contour_ref.contour) on a GIVEN frame table {c, pitch, gain}: S (513, F) -> S' (513, F')."""
    t = dtype
    St = np.ascontiguousarray(np.asarray(S, dtype=np.float32).T).astype(t)
    F = St.shape[0]
    c = np.asarray(c, dtype=np.uint32)
    C, Fp = int(c[-1]), cr.frames_of(c[-1])
    floor_t = t(np.float32(log_floor))
    out = np.empty((Fp, NB), dtype=t)
    for j in range(Fp):
        tt = min(j * 65536, C)
        i = min(int(np.searchsorted(c, tt, side="right")) - 1, F - 2)
        num, den = tt - int(c[i]), int(c[i + 1]) - int(c[i])
        w = t(np.float32(num)) / t(np.float32(den)) if t == np.float32 else t(num) / t(den)
        frame = (t(1) - w) * St[i] + w * St[i + 1]
        pj = t(pitch[i]) + w * (t(pitch[i + 1]) - t(pitch[i]))
        gj = t(gain[i]) + w * (t(gain[i + 1]) - t(gain[i]))
        out[j] = gj * frame if pj == 1 else gj * cr._pitch_frame(frame, pj, lifter, floor_t, t)
    assert out.dtype == t
    return np.ascontiguousarray(out.T)


def pitch_target(S, target, o=None, contour_points=None, dtype=np.float64):
    """The whole application in `dtype`: tracker, target, table, stage.  Returns (S', ratio, f0, stats)."""
    o = opts() if o is None else o
    _, raw, strength, _ = frames(S, o, dtype)
    f0, voiced, ratio, stats = track(raw.astype(np.float32), strength.astype(np.float32), o, target, dtype)
    F = np.asarray(S).shape[1]
    c, pt, gn = rate1_table(F) if contour_points is None else cr.table(contour_points, F)
    return apply_table(S, c, table_pitch(pt, ratio), gn, dtype=dtype), ratio, f0, stats


# ---- measuring helpers of the tests ----
def true_f0(F, f0, vibrato=0.03):
    """The instantaneous F0 of prosody_ref.voiced_signal at the centre of frame j: f0 (1 + v sin(2 pi 5 t)), t = 256 j / 22050."""
    tt = np.arange(F) * HOP / SR
    return f0 * (1.0 + vibrato * np.sin(2 * np.pi * 5.0 * tt))


def cents(a, b):
    return 1200.0 * np.log2(np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64))


def excursion_cents(f0, voiced, lo=4, hi=5):
    """Peak-to-peak excursion, in cents, of the voiced F0 over frames lo .. F - hi - 1."""
    f = np.asarray(f0, dtype=np.float64)[lo : len(f0) - hi]
    v = np.asarray(voiced)[lo : len(voiced) - hi]
    f = f[v]
    return float(1200.0 * np.log2(f.max() / f.min()))


def lower_median(x):
    x = np.sort(np.asarray(x))
    return x[(x.size - 1) // 2]
