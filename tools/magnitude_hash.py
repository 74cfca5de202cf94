"""Developer aid: the bits of everything that passes the vocoder's magnitude chain (magnitude.cpp: tracker and targets -> contour |
uniform prosody -> timbre -> SPSI initial phase, between mel -> linear and the loop), as one line per delivered array -- sha1 of
its bytes, then the F0 stats of the call, floats as exact hex -- for a fixed list of calls under three settings: the chain off,
the uniform prosody with a handle timbre, and contour + pitch target + timbre + SPSI.  Two builds of the library compute the same
bits exactly when their outputs are equal line for line (XDTTS_LIB selects the build):

  python tools/magnitude_hash.py > new.txt
  XDTTS_LIB=path/to/other/libxdtts_hip.so python tools/magnitude_hash.py > old.txt && diff old.txt new.txt

The calls: every *_linear / *_linear_batch / spsi_phase* hook on a ragged five; infer_prosody, infer_contour, infer_pitch_target
and their batch forms; one synthesize, one synthesize_batch, one synthesize_sequence and one synthesize_document over the small
golden model (tests/golden/tacotron2_small.npz: its weight seed, and its ids as the first utterance) with what the setting allows."""
import hashlib, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
wl = importlib.import_module("xd-tts_amd.workloads")

FRAMES = (40, 2, 25, 123, 24)  # the ragged five: two SPSI segments, the shortest, one segment and a frame, six, exactly one
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "tacotron2_small.npz"))
TIMBRE = dict(vtl=1.12, breath=0.25, seed=9)
RATES = (0.5, 2.0, 1.0, 1.3, 0.8)  # an identity in the middle
PITCHES = (1.2, 0.8, 1.0, 1.0, 1.1)


def mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


def magnitude(rng, F, f0):
    """a harmonic comb of f0 Hz under a smooth envelope, with a little noise: something the tracker finds a pitch in"""
    hz = np.arange(513) * 22050.0 / 1024.0
    comb = 0.05 + np.exp(-0.5 * (((hz[:, None] / f0 + 0.5) % 1.0 - 0.5) * f0 / 25.0) ** 2)
    env = np.exp(-hz / 3000.0)[:, None] * (1.0 + 0.3 * np.sin(np.arange(F) / 5.0))[None, :]
    return (comb * env * rng.uniform(0.9, 1.1, size=(513, F))).astype(np.float32)


def contour(u):
    return pkg.ProsodyContour([(0.0, RATES[u], 0.9, 1.0), (0.5, 1.0, 1.1, 0.7), (1.0, 1.0 / RATES[u], 1.25, 1.2)])


def target(u):
    return (pkg.PitchTarget(hz=180.0), pkg.PitchTarget(factor=1.1, range=0.5), pkg.PitchTarget(), pkg.PitchTarget(hz=110.0, range=1.5),
            pkg.PitchTarget(factor=0.9))[u]


def fields(s):
    vals = [getattr(s, name) for name, _ in s._fields_]
    return "/".join(x.hex() if isinstance(x, float) else str(x) for x in vals)


def line(tag, a, f0=()):
    a = np.ascontiguousarray(a)
    print("%-40s %s n=%-7d %s f0=[%s]" % (tag, a.dtype, a.size, hashlib.sha1(a.tobytes()).hexdigest(), ",".join(fields(s) for s in f0)))


def lines(tag, arrays, f0=()):
    for u, a in enumerate(arrays):
        line("%s[%d]" % (tag, u), a, f0 if u == 0 else ())


def hooks(setting, voc):
    rng = np.random.default_rng(31)
    Ss = [magnitude(rng, F, 90.0 + 40.0 * u) for u, F in enumerate(FRAMES)]
    n = len(Ss)
    pros = [pkg.Prosody(rate=RATES[u], pitch=PITCHES[u]) for u in range(n)]
    cons = [contour(u) for u in range(n)]
    tgts = [target(u) for u in range(n)]
    tims = [pkg.Timbre(vtl=1.0 + 0.05 * u, breath=0.1 * u, seed=3 + u) for u in range(n)]  # (the first is the identity)
    for u in range(n):
        if FRAMES[u] >= 2 or (RATES[u] == 1.0 and PITCHES[u] == 1.0):
            line("%s prosody_linear[%d]" % (setting, u), voc.prosody_linear(Ss[u], pros[u]))
        line("%s contour_linear[%d]" % (setting, u), voc.contour_linear(Ss[u], cons[u]))
        raw, strength, f0, st = voc.f0_linear(Ss[u])
        line("%s f0_linear[%d]" % (setting, u), np.concatenate([raw, strength, f0]), [st])
        out, ratio, st = voc.pitch_target_linear(Ss[u], tgts[u], cons[u] if u % 2 else None)
        line("%s pitch_target_linear[%d]" % (setting, u), np.concatenate([out.ravel(), ratio]), [st])
        line("%s timbre_linear[%d]" % (setting, u), voc.timbre_linear(Ss[u], tims[u]))
        turns, ang = voc.spsi_phase(Ss[u])
        line("%s spsi_phase[%d]" % (setting, u), np.concatenate([turns.ravel(), ang.ravel().view(np.uint32)]))
    lines("%s prosody_linear_batch" % setting, voc.prosody_linear_batch(Ss, pros))
    lines("%s contour_linear_batch" % setting, voc.contour_linear_batch(Ss, cons))
    raw, strength, f0, st = voc.f0_linear_batch(Ss)
    lines("%s f0_linear_batch" % setting, [np.concatenate(x) for x in zip(raw, strength, f0)], st)
    outs, ratios, st = voc.pitch_target_linear_batch(Ss, tgts, [cons[u] if u % 2 else None for u in range(n)])
    lines("%s pitch_target_linear_batch" % setting, [np.concatenate([o.ravel(), r]) for o, r in zip(outs, ratios)], st)
    lines("%s timbre_linear_batch" % setting, voc.timbre_linear_batch(Ss, tims))
    turns, angs = voc.spsi_phase_batch(Ss)
    lines("%s spsi_phase_batch" % setting, [np.concatenate([t.ravel(), a.ravel().view(np.uint32)]) for t, a in zip(turns, angs)])


def run(setting, model):
    voc = pkg.create_griffin_lim(iters=4, seed=5)
    if setting != "off":
        voc.set_timbre(pkg.Timbre(**TIMBRE))
    if setting == "contour":
        voc.set_phase_init(1)
    hooks(setting, voc)
    rng = np.random.default_rng(20)
    mels = [mel(rng, F) for F in FRAMES]
    n = len(mels)
    pros = [pkg.Prosody(rate=RATES[u], pitch=PITCHES[u]) for u in range(n)]
    cons = [contour(u) for u in range(n)]
    tgts = [target(u) for u in range(n)]
    line("%s infer" % setting, voc.infer(mels[0]), voc.last_f0())
    lines("%s infer_batch" % setting, voc.infer_batch(mels), voc.last_f0())
    for u in range(n):
        line("%s infer_prosody[%d]" % (setting, u), voc.infer_prosody(mels[u], pros[u]), voc.last_f0())
        line("%s infer_contour[%d]" % (setting, u), voc.infer_contour(mels[u], cons[u]), voc.last_f0())
        line("%s infer_pitch_target[%d]" % (setting, u), voc.infer_pitch_target(mels[u], tgts[u], cons[u] if u % 2 else None), voc.last_f0())
    lines("%s infer_batch prosody" % setting, voc.infer_batch(mels, prosody=pros), voc.last_f0())
    lines("%s infer_batch contour" % setting, voc.infer_batch(mels, contour=cons), voc.last_f0())
    lines("%s infer_batch_pitch_target" % setting, voc.infer_batch_pitch_target(mels, tgts, [cons[u] if u % 2 else None for u in range(n)]), voc.last_f0())
    lines("%s infer_batch_pitch_target identities" % setting, voc.infer_batch_pitch_target(mels[:2], [pkg.PitchTarget()] * 2), voc.last_f0())
    ids = [GOLDEN["ids"].astype(np.int64)] + [wl.synth_ids(k, seed=71 + i) for i, k in enumerate([33, 52])]
    o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
    kw1 = {"off": {}, "uniform": dict(prosody=pros[0]), "contour": dict(contour=cons[1], target=tgts[0])}[setting]
    kwn = {"off": {}, "uniform": dict(prosody=pros[:3]), "contour": dict(contour=[cons[0], None, cons[3]], target=tgts[:3])}[setting]
    seq = None if setting == "off" else pros[:3]
    _m, a = pkg.synthesize(model, voc, ids[0], opts=o, **kw1)
    line("%s synthesize" % setting, a, voc.last_f0())
    _m, audios = pkg.synthesize_batch(model, voc, [[x] for x in ids], opts=o, want_mels=False, **kwn)
    lines("%s synthesize_batch" % setting, audios, voc.last_f0())
    _m, audios = pkg.synthesize_sequence(model, voc, ids, None, opts=o, want_mels=False, prosody=seq)
    lines("%s synthesize_sequence" % setting, audios, voc.last_f0())
    _m, pcm, off = pkg.synthesize_document(model, voc, ids, (0, 441, 0, 100), pkg.StreamOpts(format=1, level=0), opts=o, want_mels=False, prosody=seq)
    line("%s synthesize_document" % setting, pcm, voc.last_f0())
    print("%-40s offsets %s" % ("", list(off)))
    voc.close()


def main():
    if pkg.device_count() < 1:
        sys.exit("magnitude_hash.py needs a HIP device")
    model = pkg.Tacotron2.synthetic(seed=int(GOLDEN["weight_seed"]))
    for setting in ("off", "uniform", "contour"):
        run(setting, model)
    model.close()


if __name__ == "__main__":
    main()
