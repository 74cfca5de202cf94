"""The timbre stage (vocal-tract length and breathiness in the vocoder) through the product alone:
err(gpu) and d32 of k_timbre against the fp64 restatement (tests/timbre_ref.py) for every case of the GPU test, the three
properties the stage exists for on the device's own output (the pitch period under vtl, the cepstral-peak ratio under breath,
the power centroid of an envelope bump), the voiced fraction xdtts_griffinlim_f0_audio reports for the audio of 30 iterations
at breath 0 / 0.5 / 1, and the device time of k_timbre at F = 800 and for a ragged batch of 32 utterances of F = 25 next to the
pitch branch of k_prosody / k_prosody_batch on the same magnitudes.

  python tools/timbre_check.py                       # prints the table
  python tools/timbre_check.py > profiles/timbre.txt
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/timbre_check.py --timing-only     # the kernels' own times
"""
import argparse, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import prosody_ref as pr  # the voiced signal
import timbre_ref as tr   # the restatement, the properties


def accuracy(voc):
    print("k_timbre against the fp64 restatement: max |x - ref64| / max(ref64, log_floor); d32 = the fp32 restatement's; rule 4 d32 + 2e-5")
    print("  %3s %5s %6s %-16s | %10s %10s %s" % ("F", "vtl", "breath", "", "err(gpu)", "d32", ""))
    cases = [(F, vtl, breath, {}) for vtl, breath in tr.CASES for F in (1, 3, 5, 37)]
    cases += [(9, 0.7, 0.4, kw) for kw in (dict(lifter=1), dict(lifter=255), dict(log_floor=1e-3))]
    for F, vtl, breath, kw in cases:
        S = tr.random_magnitude(F, seed=200 + F)
        ref = tr.timbre(S, vtl=vtl, breath=breath, seed=9, **kw)
        fl = kw.get("log_floor", 1e-5)
        d32 = tr.rel_err(tr.timbre(S, vtl=vtl, breath=breath, seed=9, dtype=np.float32, **kw), ref, fl)
        dg = tr.rel_err(voc.timbre_linear(S, pkg.Timbre(vtl=vtl, breath=breath, seed=9, **kw)), ref, fl)
        print("  %3d %5.2f %6.2f %-16s | %10.3e %10.3e %s" % (F, vtl, breath, " ".join("%s %g" % kv for kv in kw.items()), dg, d32,
                                                             "ok" if dg <= 4 * d32 + 2e-5 else "OVER"))


def properties(voc):
    print("the three properties on the device's output (voiced signal F = 48: pitch period 157 samples; envelope bump, sigma 20 bins):")
    tr.check_properties(lambda S, vtl, breath: voc.timbre_linear(S, pkg.Timbre(vtl=vtl, breath=breath)), say=lambda s: print("  " + s))


def voiced_fraction(voc):
    y = pr.voiced_signal(256 * 47)
    S, _ = voc.analyze(y)
    print("audio of 30 iterations from the voiced signal's own magnitude, through xdtts_griffinlim_f0_audio (default options):")
    for breath in (0.0, 0.5, 1.0):
        voc.set_seed(3)
        St = S if breath == 0.0 else voc.timbre_linear(S, pkg.Timbre(breath=breath))
        audio = voc.infer_linear(St, iters=30)
        _, strength, _, st = voc.f0_audio(audio)
        print("  breath %.1f: %2d of %2d frames voiced (%.2f), median %.1f Hz, median cepstral strength %.3f" % (
            breath, st.n_voiced, st.n_frames, st.n_voiced / max(st.n_frames, 1), st.median_hz, float(np.median(strength))))


def best_us(call, voc, n=5):
    call()  # warm: buffers
    best = 1e30
    for _ in range(n):
        call()
        best = min(best, voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return best


def timing(voc, F, n_utt=32, Fr=25):
    rng = np.random.default_rng(1)
    S = np.exp(rng.uniform(-9.0, 0.0, size=(513, F))).astype(np.float32)
    print("device time of the stage alone at F = %d (best of 5, HIP events on the handle's stream around the one launch):" % F)
    pro = best_us(lambda: voc.prosody_linear(S, pkg.Prosody(pitch=1.25)), voc)
    print("  %-32s %7.1f us" % ("k_prosody pitch 1.25", pro))
    for name, kw in (("vtl 1.25", dict(vtl=1.25)), ("breath 0.5", dict(breath=0.5)), ("vtl 1.25 + breath 0.5", dict(vtl=1.25, breath=0.5))):
        us = best_us(lambda: voc.timbre_linear(S, pkg.Timbre(**kw)), voc)
        print("  %-32s %7.1f us   = %.2f x k_prosody" % ("k_timbre " + name, us, us / pro))
    Ss = [np.exp(rng.uniform(-9.0, 0.0, size=(513, Fr))).astype(np.float32) for _ in range(n_utt)]
    print("the ragged stage, %d utterances of F = %d in one launch (best of 5):" % (n_utt, Fr))
    pro = best_us(lambda: voc.prosody_linear_batch(Ss, [pkg.Prosody(pitch=1.25)] * n_utt), voc)
    print("  %-32s %7.1f us" % ("k_prosody_batch pitch 1.25", pro))
    for name, kw in (("vtl 1.25", dict(vtl=1.25)), ("vtl 1.25 + breath 0.5", dict(vtl=1.25, breath=0.5))):
        ts = [pkg.Timbre(seed=u, **kw) for u in range(n_utt)]
        us = best_us(lambda: voc.timbre_linear_batch(Ss, ts), voc)
        outs = voc.timbre_linear_batch(Ss, ts)
        same = all(np.array_equal(outs[u], voc.timbre_linear(Ss[u], ts[u])) for u in (0, 1, n_utt - 1))
        print("  %-32s %7.1f us   = %.2f x k_prosody_batch   outputs against the single call: %s" % (
            "k_timbre " + name, us, us / pro, "bit for bit" if same else "DIFFER"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=800, help="frames of the timed magnitude (the headline utterance has 800)")
    ap.add_argument("--timing-only", action="store_true", help="the timed launches alone (for a kernel trace)")
    a = ap.parse_args()
    voc = pkg.create_griffin_lim(seed=3)
    voc.set_opts(output_normalise=0)
    if not a.timing_only:
        accuracy(voc)
        properties(voc)
        voiced_fraction(voc)
    timing(voc, a.frames)


if __name__ == "__main__":
    main()
