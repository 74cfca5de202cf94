"""Spectral convergence of the vocoder against its own target, through the product alone (no oracle): for a mel (.npy, 80 x F),
the headline utterance's mel (configs[1], F = 800) or the config-5 chirps, || |STFT(audio_k)| - S || / || S || after
k = 1, 2, 5, 10, 20, 30, 60, 120 iterations (infer_linear + spectral_convergence), and the device time of the analysis calls
next to one Griffin-Lim iteration at the same F.

  python tools/gl_convergence.py                 # headline mel and F = 1000 chirps
  python tools/gl_convergence.py --mel m.npy     # a mel of your own
  python tools/gl_convergence.py --chirps 200    # chirps of another length
  python tools/gl_convergence.py --phase-init both   # the seeded random start beside SPSI (phase_init 1): both columns per
                                                     # iteration count, the SPSI stage's device time, the iteration count at
                                                     # which the random start catches up, and the ragged stage on a 32-utterance batch
"""
import argparse, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")

ITERS = (1, 2, 5, 10, 20, 30, 60, 120)


def chirps(n):
    """BASELINE.md config-5 signal: five linear chirps 100 Hz - 7 kHz plus a little noise."""
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(3)
    T = t[-1] if n > 1 else 1.0
    y = sum(0.15 * np.sin(2 * np.pi * (f0 + 0.5 * (f1 - f0) * t / T) * t) for f0, f1 in ((100, 900), (400, 2500), (1200, 4000), (3000, 5500), (5000, 7000)))
    return (y + 0.01 * rng.standard_normal(n)).astype(np.float32)


def headline_mel():
    wl = importlib.import_module("xd-tts_amd.workloads")
    model = pkg.Tacotron2.synthetic(seed=wl.WEIGHT_SEED, rec_scale=1.0)
    ids, chunks, _steps = wl.config2(pkg)
    sp = np.cumsum([len(c) for c in chunks]).astype(np.int64)
    mel = model.infer(ids, splits=sp, opts=pkg.default_opts(fixed_frames_per_id=wl.FRAMES_PER_ID, dropout_seed=0, item_base=0))
    model.close()
    return np.array(mel)


BREAK_EVEN = (1, 2, 5, 10, 20, 30, 60)
BREAK_EVEN_MAX = 240  # iterations of the random start tried for a break-even


def converge(voc, S, k, mode):
    voc.set_phase_init(mode)
    c, _ = voc.spectral_convergence(voc.infer_linear(S, iters=k), S)
    voc.set_phase_init(0)
    return c


def report_both(voc, S):
    """Random start beside SPSI: the two columns, the stage's device time in iterations' worth, and for each budget K the
    first iteration count at which the random start is as close as SPSI after K."""
    rand = {}
    spsi = {k: converge(voc, S, k, 1) for k in ITERS}
    for k in ITERS:
        rand[k] = converge(voc, S, k, 0)
        print("  %3d iterations: spectral convergence random %.5f   spsi %.5f   ratio %.3f" % (k, rand[k], spsi[k], spsi[k] / rand[k]))
    stage = []
    for _ in range(5):
        voc.spsi_phase(S)
        stage.append(voc.last_timings()["mel_to_linear_ms"])  # (after the hook: the stage alone)
    voc.set_phase_init(1)
    ms = []
    for _ in range(3):
        voc.infer_linear(S, iters=ITERS[-1])
        ms.append(voc.last_timings()["iterations_ms"])
    voc.set_phase_init(0)
    per_iter_us = min(ms) * 1e3 / (ITERS[-1] + 1)
    stage_us = min(stage) * 1e3
    stage_iters = stage_us / per_iter_us
    print("  SPSI stage: %.1f us (best of 5, device) = %.1f iterations' worth at %.2f us per iteration" % (stage_us, stage_iters, per_iter_us))
    def rand_at(n):
        if n not in rand:
            rand[n] = converge(voc, S, n, 0)
        return rand[n]

    for k in BREAK_EVEN:
        n = next((n for n in range(1, BREAK_EVEN_MAX + 1) if rand_at(n) <= spsi[k]), None)
        if n is None:
            print("  break-even K = %2d: spsi %.5f is not reached by the random start within %d iterations" % (k, spsi[k], BREAK_EVEN_MAX))
        else:
            print("  break-even K = %2d: spsi %.5f is reached by the random start after %d iterations; stage + K = %.1f iterations' worth" % (
                k, spsi[k], n, stage_iters + k))


def report_ragged(voc):
    """The ragged stage alone on the 32-utterance vocoder batch of tools/vocoder_batch.py (500 .. 1000 frames each)."""
    rng = np.random.default_rng(4)
    Fs = [int(f) for f in rng.integers(500, 1000, size=32)]
    mags = [voc.mel_to_linear(rng.uniform(-7.0, -1.0, size=(80, F)).astype(np.float32)) for F in Fs]
    ms = []
    for _ in range(5):
        voc.spsi_phase_batch(mags)
        ms.append(voc.last_timings()["mel_to_linear_ms"])
    print("ragged SPSI stage: 32 utterances, %d frames: %.1f us (best of 5, device)" % (sum(Fs), min(ms) * 1e3))


def report(voc, name, S, phase_init="0"):
    F = S.shape[1]
    print("%s: F = %d, target || S || = %.4e" % (name, F, float(np.linalg.norm(S.astype(np.float64)))))
    if phase_init == "both":
        report_both(voc, S)
    else:
        for k in ITERS:
            c = converge(voc, S, k, int(phase_init))
            print("  %3d iterations: spectral convergence %.5f" % (k, c))
    k = ITERS[-1]
    ms = []
    for _ in range(3):
        audio = voc.infer_linear(S, iters=k)
        ms.append(voc.last_timings()["iterations_ms"])
    per_iter_us = min(ms) * 1e3 / (k + 1)
    an, sc = [], []
    for _ in range(5):
        voc.analyze(audio)
        an.append(voc.analysis_timings())
        voc.spectral_convergence(audio, S)
        sc.append(voc.analysis_timings())
    best = lambda rows, key: min(r[key] for r in rows) * 1e3  # noqa: E731
    print("  analyze: magnitude %.1f us, mel projection + compression + layouts %.1f us, total %.1f us (best of 5, device)" % (
        best(an, "magnitude_ms"), best(an, "projection_ms"), best(an, "total_ms")))
    print("  spectral_convergence: magnitude %.1f us, distance %.1f us, total %.1f us (best of 5, device)" % (
        best(sc, "magnitude_ms"), best(sc, "projection_ms"), best(sc, "total_ms")))
    print("  one Griffin-Lim iteration at this F: %.2f us (%d iterations + final ISTFT, best of 3)" % (per_iter_us, k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mel", help="a (80, F) .npy mel in the handle's conventions (natural-log)")
    ap.add_argument("--chirps", type=int, help="frames of the chirp signal")
    ap.add_argument("--phase-init", choices=("0", "1", "both"), default="0", help="the initial phase: 0 seeded random, 1 SPSI, both side by side")
    a = ap.parse_args()
    voc = pkg.create_griffin_lim(seed=3)
    voc.set_opts(output_normalise=0)
    if a.mel:
        report(voc, a.mel, voc.mel_to_linear(np.load(a.mel)), a.phase_init)
    if a.chirps:
        report(voc, "chirps", voc.analyze(chirps(256 * (a.chirps - 1)), want_mel=False)[0], a.phase_init)
    if not a.mel and not a.chirps:
        report(voc, "headline mel (configs[1])", voc.mel_to_linear(headline_mel()), a.phase_init)
        report(voc, "chirps (configs[4])", voc.analyze(chirps(256 * 999), want_mel=False)[0], a.phase_init)
    if a.phase_init == "both":
        report_ragged(voc)


if __name__ == "__main__":
    main()
