"""The silence stage of the delivery chain (include/xdtts.h: xdtts_silence) restated in numpy with serial loops, for the CPU and
GPU tests: the host integers of a rate, the per-window decisions, the gather with its fades and the stats.  Everything is
integers and comparisons but for two things: tfac = (float) pow(10, threshold_db / 20), the definition's one libm call, which
the caller takes from xdtts_silence_plan and hands in; and the fade gains, which stream_ref.fade_table restates bit for bit.
Also the crafted signals both test files run on."""
import math

import numpy as np

import stream_ref

F32 = np.float32
FIELDS = ("threshold_db", "min_sound_ms", "lead_ms", "trail_ms", "max_pause_ms", "fade_ms")
DEFAULT = dict(threshold_db=-40.0, min_sound_ms=20.0, lead_ms=50.0, trail_ms=100.0, max_pause_ms=0.0, fade_ms=2.0)
RANGES = dict(threshold_db=(-96.0, -6.0), min_sound_ms=(0.0, 500.0), lead_ms=(0.0, 10000.0), trail_ms=(0.0, 10000.0),
              max_pause_ms=(20.0, 60000.0), fade_ms=(0.0, 2.5))   # (max_pause_ms: 0 is a setting too, nothing else below 20)
STATS = ("n_in", "n_out", "lead_cut", "trail_cut", "pause_cut", "n_cuts", "peak", "any_sound")
RATES = (8000, 11025, 16000, 22050, 44100, 48000, 96000)
TILE = 4096


def settings(**kw):
    return dict(DEFAULT, **kw)


def win(ms):
    return int(math.floor(float(F32(ms)) / 5.0 + 0.5))


def plan(rate, s, tfac):
    """the host integers; tfac: from xdtts_silence_plan"""
    W = rate // 200
    return dict(W=W, min_w=win(s["min_sound_ms"]), lead_w=win(s["lead_ms"]), trail_w=win(s["trail_ms"]), pause_w=win(s["max_pause_ms"]),
                fade=min(W // 2, int(math.floor(float(F32(s["fade_ms"])) * rate / 1000.0 + 0.5))), tfac=F32(tfac))


def decisions(x, p):
    """(keep, sound, P) per window, steps 1 to 5 with serial loops"""
    x = np.asarray(x, dtype=np.float32)
    n, W = x.size, p["W"]
    nw = -(-n // W)
    pw = [F32(np.max(np.abs(x[w * W:min(n, (w + 1) * W)]))) for w in range(nw)]
    P = F32(max(pw))
    thr = F32(P * p["tfac"])
    a0 = [bool(v > thr) for v in pw]
    a = [False] * nw
    w = 0
    while w < nw:                      # maximal runs of candidates
        if not a0[w]:
            w += 1
            continue
        e = w
        while e < nw and a0[e]:
            e += 1
        if e - w >= max(p["min_w"], 1):
            for k in range(w, e):
                a[k] = True
        w = e
    keep = [False] * nw
    sound = [w for w in range(nw) if a[w]]
    if not sound:
        for w in range(min(nw, max(1, p["lead_w"] + p["trail_w"]))):
            keep[w] = True
        return keep, a, P
    A, Z, pz = sound[0], sound[-1], p["pause_w"]
    for w in range(nw):
        if a[w]:
            keep[w] = True
        elif w < A:
            keep[w] = A - w <= p["lead_w"]
        elif w > Z:
            keep[w] = w - Z <= p["trail_w"]
        else:
            l = max(k for k in sound if k < w)
            r = min(k for k in sound if k > w)
            keep[w] = pz == 0 or w - l <= pz - pz // 2 or r - w <= pz // 2
    return keep, a, P


def reference(x, p):
    """(out, stats as a tuple in the order of STATS), steps 6 and 7"""
    x = np.asarray(x, dtype=np.float32)
    n, W, fade = x.size, p["W"], p["fade"]
    nw = -(-n // W)
    keep, a, P = decisions(x, p)
    T = stream_ref.fade_table(fade) if fade else np.zeros(0, dtype=np.float32)
    sound = [w for w in range(nw) if a[w]]
    out, cut, n_cuts = [], [0, 0, 0], 0
    for w in range(nw):
        seg = x[w * W:min(n, (w + 1) * W)].copy()
        if not keep[w]:
            kind = 1 if not sound or w > sound[-1] else (0 if w < sound[0] else 2)
            cut[kind] += seg.size
            continue
        if w > 0 and not keep[w - 1]:
            n_cuts += 1
            m = min(fade, seg.size)
            seg[:m] = seg[:m] * T[:m]
        if w < nw - 1 and not keep[w + 1]:
            n_cuts += 1
            m = min(fade, seg.size)
            seg[seg.size - m:] = seg[seg.size - m:] * T[:m][::-1]
        out.append(seg)
    y = np.concatenate(out)
    return y, (n, y.size, cut[0], cut[1], cut[2], n_cuts, float(P), 1 if sound else 0)


# ---- crafted signals ---------------------------------------------------------------------------------------------------------

def craft(rate, segs, seed=0):
    """segs: ("sine", samples, amplitude) | ("zero", samples) | ("noise", samples, amplitude).  A 440 Hz sine with a phase that
    keeps its first sample away from zero: every 5 ms window of a burst holds more than two periods, so its peak is the
    amplitude's within a fraction of a per cent."""
    rng = np.random.Generator(np.random.PCG64(4000 + seed))
    parts = []
    for s in segs:
        k = int(s[1])
        if s[0] == "sine":
            parts.append(s[2] * np.sin(2.0 * np.pi * 440.0 * np.arange(k) / rate + 0.9))
        elif s[0] == "noise":
            parts.append(s[2] * rng.uniform(-1.0, 1.0, size=k))
        else:
            parts.append(np.zeros(k))
    return np.concatenate(parts).astype(np.float32)


def cases():
    """[(name, rate, settings, x)]: what test_silence_cpu.py holds against the restatement and test_gpu_silence.py against
    xdtts_silence_reference.  W = 110 at 22050; the defaults are min_w 4, lead_w 10, trail_w 20, fade 44."""
    out = []
    Q, W = 22050, 110
    for n in (1, W - 1, W, W + 1, 4096, 4097):
        out.append(("n=%d" % n, Q, settings(), craft(Q, [("sine", n, 0.5)])))
    out.append(("zeros", Q, settings(), np.zeros(5000, dtype=np.float32)))
    out.append(("all sound", Q, settings(), craft(Q, [("sine", 10000, 0.9)])))
    # a click of min_w - 1 windows, one of exactly min_w, then speech; zeros between them
    clicks = [("zero", 30 * W), ("sine", 3 * W, 0.9), ("zero", 30 * W), ("sine", 4 * W, 0.6), ("zero", 30 * W), ("sine", 20 * W, 0.3), ("zero", 41 * W + 7)]
    out.append(("clicks", Q, settings(), craft(Q, clicks)))
    # pauses of exactly pause_w and of pause_w + 1 windows: zeros, and noise 20 dB under a -30 dB threshold
    for name, ms in (("even", 100.0), ("odd", 105.0)):
        pz = win(ms)
        zs = [("zero", 13 * W), ("sine", 20 * W, 0.9), ("zero", pz * W), ("sine", 20 * W, 0.05), ("zero", (pz + 1) * W), ("sine", 20 * W, 0.4),
              ("zero", 3 * pz * W), ("sine", 9 * W, 0.2), ("zero", 25 * W + 50)]
        out.append(("pauses %s" % name, Q, settings(threshold_db=-30.0, max_pause_ms=ms), craft(Q, zs)))
        amp = 0.9 * 10.0 ** (-50.0 / 20.0)
        ns = [(("noise", s[1], amp) if s[0] == "zero" else s) for s in zs]
        out.append(("pauses %s noise" % name, Q, settings(threshold_db=-30.0, max_pause_ms=ms), craft(Q, ns, seed=1)))
    short = [("zero", 3 * W), ("sine", 30 * W, 0.7), ("zero", 5 * W), ("sine", 8 * W, 0.7), ("zero", 6 * W + 3)]
    out.append(("lead and trail past the ends", Q, settings(lead_ms=10000.0, trail_ms=10000.0), craft(Q, short)))
    out.append(("lead = trail = 0", Q, settings(lead_ms=0.0, trail_ms=0.0, max_pause_ms=20.0), craft(Q, clicks)))
    out.append(("fade = 0", Q, settings(fade_ms=0.0, max_pause_ms=40.0), craft(Q, clicks)))
    # the last window, 10 samples, is the only sound and shorter than the fade; the window in front of it is dropped
    out.append(("short last window", Q, settings(min_sound_ms=0.0, lead_ms=0.0), craft(Q, [("zero", 40 * W), ("sine", 10, 0.8)])))
    # more windows than k_sil_plan's workgroup has lanes: 1200 windows, chunks of 256 with carries across every boundary
    long_segs, k = [], 0
    while sum(s[1] for s in long_segs) < 1200 * W:
        long_segs += [("sine", (37 + 11 * (k % 5)) * W, 0.1 + 0.2 * (k % 4)), ("zero" if k % 2 else "noise", (9 + 17 * (k % 7)) * W, 0.7 * 10.0 ** (-50.0 / 20.0))]
        k += 1
    x = craft(Q, long_segs, seed=2)[:1200 * W]
    out.append(("1200 windows", Q, settings(threshold_db=-30.0, max_pause_ms=200.0), x))   # (peak 0.7: the noise is 20 dB under the threshold)
    # 11025 Hz, W = 55: 4096 = 74 W + 26, the windows straddle every tile boundary
    q, w = 11025, 55
    strad = [("zero", 20 * w), ("sine", 150 * w, 0.5), ("zero", 70 * w), ("sine", 100 * w, 0.25), ("zero", 33 * w + 17)]
    out.append(("11025 straddle", q, settings(max_pause_ms=150.0), craft(q, strad)))
    out.append(("8000", 8000, settings(max_pause_ms=60.0, fade_ms=2.5), craft(8000, [("zero", 900), ("sine", 3000, 0.6), ("noise", 2000, 0.001), ("sine", 2500, 0.9), ("zero", 1500)], seed=3)))
    out.append(("48000", 48000, settings(max_pause_ms=30.0), craft(48000, [("zero", 5000), ("sine", 9000, 0.6), ("zero", 12000), ("sine", 7001, 0.9), ("zero", 9000)])))
    return out
