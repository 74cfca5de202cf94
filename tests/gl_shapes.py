"""Shared by test_gl_shapes_cpu.py and test_gpu_griffinlim_shapes.py: the Griffin-Lim engine and
work-split rules restated in plain Python, the frame counts that reach every shape they produce, the
input of the sweep, and the two metrics that look at one hop / one frame at a time.

The rules restated here (csrc/gl_plan.h: gl_persistent_plan and the batch packer; csrc/griffinlim.hip: glp_fstart,
launch_gl_iterate):

  F < 16                      two kernels per iteration (reflect padding folds more than once)
  tf = max(4, ceil(F / n_cu)) frames per workgroup of the persistent kernel; tf > GLP_TF_MAX -> launch engine
  nblk = ceil(F / tf)         workgroups; workgroup b owns floor((b+1) F / nblk) - floor(b F / nblk) frames
  launch engine               k_gl_fused<4>: ceil(F / 4) blocks of 4 frames, the last one partial
  batch                       the same split with tf = 4 or 8 whatever the CU count; an utterance whose split
                              leaves a workgroup fewer than 3 frames (or F < 16) runs on its own
"""
import numpy as np

HOP = 256
N_BINS = 513
GLP_TF_MAX = 8    # csrc/gl_plan.h
TINY_BELOW = 16   # gl_persistent_plan: "if (F < 16) return false"; launch_gl_iterate: "if (g.F >= 16)"
MIN_OWN = 3       # the edge sums of k_gl_persistent reach three frames back

# the sweep of test_gpu_griffinlim_shapes.py, one list per test
SWEEP_DEFAULT = (10, 15, 16, 17, 18, 19, 21, 37, 203, 1024, 1026, 1281, 1537, 1793, 2048, 2049)
SWEEP_LAUNCH = (16, 17, 19, 203, 1026, 2049)
SWEEP_STEP = (15, 16, 17, 203, 1026, 1793, 2049)
SWEEP_SEEDED = (17, 1026)
BATCH_FRAMES = (16, 17, 19, 37, 64, 203, 5)


def even_split(F, nblk):
    """Own frames of workgroups 0 .. nblk-1 (glp_fstart)."""
    return [((b + 1) * F) // nblk - (b * F) // nblk for b in range(nblk)]


def plan(F, n_cu=256):
    """(engine, TF, own frames per workgroup) of a single call of F frames on a device of n_cu CUs.
    engine: "tiny" (two kernels per iteration), "p4" / "p8" (k_gl_persistent<4> / <8>, TF = threads / 64
    of the launch) or "launch" (k_gl_fused<4>, TF = 4)."""
    if F < TINY_BELOW:
        return "tiny", 4, [min(4, F - f) for f in range(0, F, 4)]
    launch = ("launch", 4, [min(4, F - f) for f in range(0, F, 4)])
    tf = max(4, -(-F // n_cu))
    if tf > GLP_TF_MAX:
        return launch
    nblk = -(-F // tf)
    if nblk > n_cu or F // nblk < MIN_OWN:
        return launch
    return ("p4" if tf == 4 else "p8"), tf, even_split(F, nblk)


def batch_split(F, tf, n_cu=256):
    """Own frames per workgroup of an utterance of F frames inside a batch launch of tf-frame workgroups
    (tf = 4 or 8), or None when the packer leaves the utterance to the single call's engine."""
    nblk = -(-F // tf)
    if F < TINY_BELOW or nblk > n_cu or F // nblk < MIN_OWN:
        return None
    return even_split(F, nblk)


def shape_class(F, n_cu=256):
    """The name of the shape a frame count exercises; test_gl_shapes_cpu.py asks for every one of them."""
    engine, tf, own = plan(F, n_cu)
    if engine in ("tiny", "launch"):
        return engine
    if engine == "p4":
        if min(own) == 4:
            return "p4-all4"
        # (the floor split gives workgroup 0 floor(F / nblk) = 3 frames and the last one ceil(F / nblk) = 4 whenever
        # 4 does not divide F, so "a 3 at the last workgroup only" cannot occur: test_gl_shapes_cpu.py pins that)
        threes = [b for b, n in enumerate(own) if n == 3]
        if threes == [len(own) - 1]:
            return "p4-3-last"
        return "p4-3-first-only" if threes == [0] else "p4-3-inside"
    return "p8-tf%d-%s" % (tf, "mixed" if min(own) != max(own) else "even")


def chirps(n):
    """Five linear chirps 100 Hz - 7 kHz plus a little noise (the BASELINE config-5 signal)."""
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(3)
    y = sum(0.15 * np.sin(2 * np.pi * (f0 + 0.5 * (f1 - f0) * t / t[-1]) * t) for f0, f1 in ((100, 900), (400, 2500), (1200, 4000), (3000, 5500), (5000, 7000)))
    return (y + 0.01 * rng.standard_normal(n)).astype(np.float32)


def chirp_S(orc, F):
    """(513, F) fp32 magnitude of the chirp signal's STFT, computed by the oracle."""
    spec = orc.stft(chirps(HOP * (F - 1)))
    return np.hypot(spec[..., 0], spec[..., 1]).astype(np.float32)


def speech_mel(F, seed):
    """(80, F) natural-log mel of speech-like range for the batch test."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 6.0)[None, :]).astype(np.float32)


def rms(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def hop_rms(a, ref):
    """RMS of a - ref inside each of the F - 1 hops of 256 samples."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    assert d.ndim == 1 and d.size % HOP == 0 and d.size > 0
    return np.sqrt(np.mean(d.reshape(-1, HOP) ** 2, axis=1))


def worst_hop(a, ref):
    """max over the hops of hop_rms: a wrong overlap at ONE workgroup boundary spoils three hops whatever
    the length of the utterance, where a whole-signal RMS dilutes it by sqrt(F / 3)."""
    return float(hop_rms(a, ref).max())


def per_frame_rel(r, ref):
    """For each frame f: ||r[:, f] - ref[:, f]|| / ||ref[:, f]|| over the 513 complex bins; r, ref are (513, F, 2)."""
    r = np.asarray(r, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert r.shape == ref.shape and r.ndim == 3 and r.shape[2] == 2
    num = np.sqrt(np.sum((r - ref) ** 2, axis=(0, 2)))
    den = np.sqrt(np.sum(ref ** 2, axis=(0, 2)))
    return num / np.maximum(den, 1e-300)
