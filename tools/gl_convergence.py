"""Spectral convergence of the vocoder against its own target, through the product alone (no oracle): for a mel (.npy, 80 x F),
the headline utterance's mel (configs[1], F = 800) or the config-5 chirps, || |STFT(audio_k)| - S || / || S || after
k = 1, 2, 5, 10, 20, 30, 60, 120 iterations (infer_linear + spectral_convergence), and the device time of the analysis calls
next to one Griffin-Lim iteration at the same F.

  python tools/gl_convergence.py                 # headline mel and F = 1000 chirps
  python tools/gl_convergence.py --mel m.npy     # a mel of your own
  python tools/gl_convergence.py --chirps 200    # chirps of another length
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


def report(voc, name, S):
    F = S.shape[1]
    print("%s: F = %d, target || S || = %.4e" % (name, F, float(np.linalg.norm(S.astype(np.float64)))))
    for k in ITERS:
        c, _ = voc.spectral_convergence(voc.infer_linear(S, iters=k), S)
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
    a = ap.parse_args()
    voc = pkg.create_griffin_lim(seed=3)
    voc.set_opts(output_normalise=0)
    if a.mel:
        report(voc, a.mel, voc.mel_to_linear(np.load(a.mel)))
    if a.chirps:
        report(voc, "chirps", voc.analyze(chirps(256 * (a.chirps - 1)), want_mel=False)[0])
    if not a.mel and not a.chirps:
        report(voc, "headline mel (configs[1])", voc.mel_to_linear(headline_mel()))
        report(voc, "chirps (configs[4])", voc.analyze(chirps(256 * 999), want_mel=False)[0])


if __name__ == "__main__":
    main()
