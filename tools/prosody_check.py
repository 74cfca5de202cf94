"""The prosody stage (speaking rate and pitch in the vocoder) through the product alone: device time of
k_prosody at F = 800 for a rate change, a pitch change and both, next to one Griffin-Lim iteration of the same run, and what the
stage does to a synthetic voiced sound (F0 of the audio before and after, true magnitude and mel path); then the ragged stage
of the batch entries: one k_prosody_batch launch for 32 utterances of F = 25 next to the same 32 as a loop of k_prosody launches;
then the contour stage (k_prosody_contour: rate, pitch and gain that vary inside an utterance) at the same F next to k_prosody
on the same branch, the host time of its table, and its ragged 32 x 25 case.

  python tools/prosody_check.py                       # prints the table
  python tools/prosody_check.py > profiles/prosody.txt
"""
import argparse, importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import prosody_ref as pr  # the voiced signal and the F0 helper of the tests


def stage_us(voc, S, p, n=5):
    """Best of n: the stage alone (HIP events around the one launch on the handle's stream)."""
    voc.prosody_linear(S, p)  # warm: buffers
    best = 1e30
    for _ in range(n):
        voc.prosody_linear(S, p)
        best = min(best, voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return best


def timing(voc, F):
    rng = np.random.default_rng(1)
    S = np.exp(rng.uniform(-9.0, 0.0, size=(513, F))).astype(np.float32)
    print("device time of the stage at F = %d (best of 5, HIP events on the handle's stream):" % F)
    rows = {}
    for name, kw in (("rate 1.25", dict(rate=1.25)), ("pitch 1.25", dict(pitch=1.25)), ("rate 1.25 + pitch 1.25", dict(rate=1.25, pitch=1.25))):
        p = pkg.Prosody(**kw)
        rows[name] = stage_us(voc, S, p)
        print("  %-24s F' = %4d  %7.1f us" % (name, pkg.prosody_frames(F, p.rate), rows[name]))
    k, ms = 120, []
    for _ in range(3):
        voc.infer_linear(S, iters=k)
        ms.append(voc.last_timings()["iterations_ms"])
    it = min(ms) * 1e3 / (k + 1)
    print("  one Griffin-Lim iteration at this F: %.2f us (%d iterations + final ISTFT, best of 3)" % (it, k))
    voc.analyze(np.zeros(256 * (F - 1), dtype=np.float32), want_mel=False)
    an = []
    for _ in range(5):
        voc.analyze(np.zeros(256 * (F - 1), dtype=np.float32), want_mel=False)
        an.append(voc.analysis_timings()["magnitude_ms"] * 1e3)
    print("  k_stft_mag at this F: %.1f us (best of 5)" % min(an))
    for name, us in rows.items():
        print("  %-24s = %.2f iterations = %.2f x k_stft_mag" % (name, us / it, us / min(an)))


def ragged(voc, n_utt=32, F=25):
    """One k_prosody_batch launch against n_utt k_prosody launches (XDTTS_PROSODY_BATCH=loop), same inputs, same stream, HIP
    events around the launches alone; best of 5 each."""
    rng = np.random.default_rng(2)
    Ss = [np.exp(rng.uniform(-9.0, 0.0, size=(513, F))).astype(np.float32) for _ in range(n_utt)]
    print("the ragged stage, %d utterances of F = %d (best of 5, HIP events on the handle's stream):" % (n_utt, F))
    for name, kw in (("rate 1.25", dict(rate=1.25)), ("pitch 1.25", dict(pitch=1.25)), ("rate 1.25 + pitch 1.25", dict(rate=1.25, pitch=1.25))):
        ps = [pkg.Prosody(**kw)] * n_utt
        us = {}
        for form in ("one launch", "loop"):
            if form == "loop":
                os.environ["XDTTS_PROSODY_BATCH"] = "loop"
            try:
                out = voc.prosody_linear_batch(Ss, ps)  # warm: buffers
                best = 1e30
                for _ in range(5):
                    voc.prosody_linear_batch(Ss, ps)
                    best = min(best, voc.last_timings()["mel_to_linear_ms"] * 1e3)
            finally:
                os.environ.pop("XDTTS_PROSODY_BATCH", None)
            us[form] = (best, out)
        same = all(np.array_equal(a, b) for a, b in zip(us["one launch"][1], us["loop"][1]))
        print("  %-24s k_prosody_batch %7.1f us   %d x k_prosody %7.1f us   ratio %.2f   outputs %s" % (
            name, us["one launch"][0], n_utt, us["loop"][0], us["loop"][0] / us["one launch"][0], "bit for bit" if same else "DIFFER"))


def contour_us(voc, S, c, n=5):
    """Best of n: (k_prosody_contour alone, the table's upload in front of it), HIP events on the handle's stream."""
    voc.contour_linear(S, c)  # warm: buffers
    best, up = 1e30, 1e30
    for _ in range(n):
        voc.contour_linear(S, c)
        t = voc.last_timings()
        best = min(best, t["mel_to_linear_ms"] * 1e3)
        up = min(up, (t["total_ms"] - t["mel_to_linear_ms"] - t["iterations_ms"]) * 1e3)
    return best, up


def contour_timing(voc, F):
    rng = np.random.default_rng(1)
    S = np.exp(rng.uniform(-9.0, 0.0, size=(513, F))).astype(np.float32)
    print("the contour stage at F = %d (k_prosody_contour alone, best of 5, HIP events on the handle's stream), k_prosody on the same branch beside it:" % F)
    cases = (("rate only: 1 -> 1.5 ramp", [(0.0, 1.0, 1.0, 1.0), (1.0, 1.5, 1.0, 1.0)], dict(rate=1.25)),
             ("pitch ramp 0.8 -> 1.25", [(0.0, 1.0, 0.8, 1.0), (1.0, 1.0, 1.25, 1.0)], dict(rate=1.0, pitch=1.25)),
             ("half the frames at pitch 1", [(0.0, 1.0, 1.0, 1.0), (0.5, 1.0, 1.0, 1.0), (0.5, 1.0, 1.25, 1.0)], dict(rate=1.0, pitch=1.25)))
    for name, points, kw in cases:
        c = pkg.ProsodyContour(points)
        us, up = contour_us(voc, S, c)
        uni = stage_us(voc, S, pkg.Prosody(**kw))
        print("  %-28s F' = %4d  %7.1f us   (table upload %5.1f us)   k_prosody %s: %7.1f us" % (
            name, pkg.prosody_contour_frames(c, F), us, up, " ".join("%s %g" % kv for kv in kw.items()), uni))
    c = pkg.ProsodyContour(cases[1][1])
    best = 1e30
    for _ in range(20):
        t0 = time.perf_counter()
        pkg.prosody_contour_table(c, F)
        best = min(best, time.perf_counter() - t0)
    print("  host: building the table for F = %d (xdtts_prosody_contour_table through ctypes, best of 20): %.1f us" % (F, best * 1e6))


def contour_ragged(voc, n_utt=32, F=25):
    rng = np.random.default_rng(2)
    Ss = [np.exp(rng.uniform(-9.0, 0.0, size=(513, F))).astype(np.float32) for _ in range(n_utt)]
    print("the ragged contour stage, %d utterances of F = %d (best of 5):" % (n_utt, F))
    for name, points in (("rate only: 1 -> 1.5 ramp", [(0.0, 1.0, 1.0, 1.0), (1.0, 1.5, 1.0, 1.0)]), ("pitch ramp 0.8 -> 1.25", [(0.0, 1.0, 0.8, 1.0), (1.0, 1.0, 1.25, 1.0)])):
        cs = [pkg.ProsodyContour(points)] * n_utt
        out = voc.contour_linear_batch(Ss, cs)  # warm: buffers
        best = 1e30
        for _ in range(5):
            voc.contour_linear_batch(Ss, cs)
            best = min(best, voc.last_timings()["mel_to_linear_ms"] * 1e3)
        same = all(np.array_equal(a, voc.contour_linear(S, cs[0])) for a, S in zip(out[:4], Ss[:4]))
        print("  %-28s k_prosody_contour %7.1f us for %d rows   first four outputs against the single call: %s" % (
            name, best, sum(o.shape[1] for o in out), "bit for bit" if same else "DIFFER"))


def effect(voc):
    y = pr.voiced_signal(256 * 47)
    S, mel = voc.analyze(y)
    mid = lambda a: pr.f0_autocorr(a[a.size // 4 : 3 * a.size // 4])  # noqa: E731
    print("what it does to a voiced sound (140 Hz, 3 %% vibrato, three formants; F = 48, 30 iterations; F0 of the middle half):")
    print("  input: %.1f Hz" % mid(y))
    f_lin, f_mel = mid(voc.infer_linear(S, iters=30)), mid(voc.infer(mel))
    print("  identity: %.1f Hz from the magnitude, %.1f Hz through the mel" % (f_lin, f_mel))
    print("  %5s %5s | %8s %10s %9s | %10s %9s" % ("rate", "pitch", "samples", "magnitude", "ratio", "mel path", "ratio"))
    for rate, pitch in ((1.0, 0.67), (1.0, 0.8), (1.0, 1.25), (1.0, 1.5), (0.7, 1.3), (1.25, 1.0), (2.0, 1.0)):
        p = pkg.Prosody(rate=rate, pitch=pitch)
        a = voc.infer_linear(voc.prosody_linear(S, p), iters=30)
        b = voc.infer_prosody(mel, p)
        print("  %5.2f %5.2f | %8d %7.1f Hz %9.4f | %7.1f Hz %9.4f" % (rate, pitch, a.size, mid(a), mid(a) / f_lin, mid(b), mid(b) / f_mel))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=800, help="frames of the timed magnitude (the headline utterance has 800)")
    a = ap.parse_args()
    voc = pkg.create_griffin_lim(seed=3)
    voc.set_opts(output_normalise=0)
    timing(voc, a.frames)
    effect(voc)
    ragged(voc)
    contour_timing(voc, a.frames)
    contour_ragged(voc)


if __name__ == "__main__":
    main()
