"""The clean-up stage (spectral subtraction with a floor and a tone curve in the vocoder) through the
product alone: k_noise_profile + k_denoise against xdtts_denoise_reference bit for bit for every frame count and quantile of the
GPU test, the properties of the definition on the device's own output, and the device time -- by HIP events on the handle's
stream, best of 5 -- at F = 800 (the headline mel) and F = 40 of each of the two kernels, the stage alone, the stage inside
infer and a ragged batch of 32, beside the timbre stage and the tracker's two launches on the same magnitude in the same run,
and the stage's share of the vocoder half.

  python tools/denoise_check.py                       # prints the table
  python tools/denoise_check.py > profiles/denoise.txt
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/denoise_check.py --timing-only     # the kernels' own times
"""
import argparse, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import denoise_ref as dr  # the crafted inputs, the scene of the properties

TONE = [(300.0, -12.0), (1000.0, 3.0), (3400.0, 0.0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def accuracy(voc):
    print("the stage alone against xdtts_denoise_reference on the crafted input, strength 2, floor -20 dB: cells that differ (of 513 F), stats")
    print("  %4s | %s" % ("F", "  ".join("q = %-4g" % q for q in (0.0, 0.1, 0.5, 1.0))))
    for F in (1, 2, 3, 15, 16, 17, 64, 65, 300, 800):
        S = dr.crafted(F)
        cells = []
        for q in (0.0, 0.1, 0.5, 1.0):
            d = pkg.Denoise(strength=2.0, quantile=q)
            want, wst = pkg.denoise_reference(S, d)
            got = voc.denoise_linear(S, d)
            ok = voc.last_denoise()[0].astuple() == wst.astuple() and np.array_equal(bits(voc.noise_profile(S, q)), bits(dr.noise(S, q)))
            cells.append("%d %s" % (int(np.count_nonzero(bits(got) != bits(want))), "ok " if ok else "STATS"))
        print("  %4d | %s" % (F, "     ".join(cells)))
    S = dr.crafted(65)
    for name, d, prof in (("tone alone", pkg.Denoise(tone=TONE), None), ("subtraction + tone", pkg.Denoise(strength=1.0, floor_db=-6.0, tone=TONE), None),
                          ("profile mode", pkg.Denoise(strength=2.0), dr.noise(dr.crafted(40, seed=1), 0.5))):
        want, _ = pkg.denoise_reference(S, d, prof)
        print("  %-20s F = 65: %d cells differ" % (name, int(np.count_nonzero(bits(voc.denoise_linear(S, d, prof)) != bits(want)))))


def properties(voc):
    print("Rayleigh noise of scale 1e-3, a three-harmonic tone of magnitude 1 over the middle 60 %, strength 2, quantile 0.5, floor -20 dB, on the device:")
    for F in (48, 96):
        S, tone = dr.tone_scene(F)
        out = voc.denoise_linear(S, pkg.Denoise(strength=2.0, quantile=0.5, floor_db=-20.0))
        st = voc.last_denoise()[0]
        fall = 20 * np.log10(np.sqrt(np.mean(out[~tone].astype(np.float64) ** 2)) / np.sqrt(np.mean(S[~tone].astype(np.float64) ** 2)))
        print("  F = %2d: noise-only rms %+.2f dB (bound -15), tone cells keep >= %.5f (bound 0.99), %d of %d cells at the floor, zeros stay zeros: %s" % (
            F, fall, float((out[tone] / S[tone]).min()), st.floored, st.cells, bool(np.all(out[S == 0] == 0))))


def best(call, read, n=5):
    call()  # warm: buffers
    vals = []
    for _ in range(n):
        call()
        vals.append(read())
    return min(vals)


def timing(voc, F, n_utt=32):
    rng = np.random.default_rng(1)
    mel = (rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32)
    S = voc.mel_to_linear(mel)
    ms0 = lambda: voc.last_timings()["mel_to_linear_ms"] * 1e3
    tot = lambda: voc.last_timings()["total_ms"] * 1e3
    d = pkg.Denoise(strength=2.0, quantile=0.5, tone=TONE)
    prof = voc.noise_profile(S, 0.5)
    print("device time at F = %d (best of 5, HIP events on the handle's stream; the stage's figures include the 16-byte stats copy behind it):" % F)
    sel = best(lambda: voc.noise_profile(S, 0.5), ms0)
    pw = best(lambda: voc.denoise_linear(S, d, prof), ms0)
    stage = best(lambda: voc.denoise_linear(S, d), ms0)
    print("  %-44s %7.1f us" % ("k_noise_profile alone (noise_profile)", sel))
    print("  %-44s %7.1f us" % ("k_denoise alone (profile mode, with tone)", pw))
    print("  %-44s %7.1f us" % ("the stage alone (selection + k_denoise)", stage))
    tim = best(lambda: voc.timbre_linear(S, pkg.Timbre(vtl=1.25)), ms0)
    trk = best(lambda: voc.f0_linear(S), tot)
    trk0 = best(lambda: voc.f0_linear(S), ms0)
    print("  %-44s %7.1f us" % ("k_timbre vtl 1.25 (same magnitude)", tim))
    print("  %-44s %7.1f us   (k_f0_frames %.1f us)" % ("the tracker's two launches (same magnitude)", trk, trk0))
    print("  the selection is %.2f x the tracker's two launches, the stage %.2f x k_timbre" % (sel / trk, stage / tim))
    voc.set_denoise(None)
    off0, offt = best(lambda: voc.infer(mel), ms0), best(lambda: voc.infer(mel), tot)
    voc.set_denoise(d)
    on0, ont = best(lambda: voc.infer(mel), ms0), best(lambda: voc.infer(mel), tot)
    voc.set_denoise(None)
    print("  %-44s %7.1f us   (mel -> linear and the chain: %.1f us on, %.1f us off)" % ("the stage inside infer (on - off)", on0 - off0, on0, off0))
    print("  the vocoder half (mel -> linear .. final ISTFT): %.1f us on, %.1f us off: the stage is %.2f %% of it" % (ont, offt, 100.0 * (on0 - off0) / ont))
    Ss = [S] * n_utt
    bat = best(lambda: voc.denoise_linear_batch(Ss, [d] * n_utt), ms0)
    outs = voc.denoise_linear_batch(Ss, [d] * n_utt)
    one = voc.denoise_linear(S, d)
    same = all(np.array_equal(bits(outs[u]), bits(one)) for u in (0, 1, n_utt - 1))
    print("  %-44s %7.1f us   = %.1f us an utterance; outputs against the single call: %s" % (
        "ragged batch of %d x F = %d" % (n_utt, F), bat, bat / n_utt, "bit for bit" if same else "DIFFER"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--timing-only", action="store_true", help="the timed launches alone (for a kernel trace)")
    a = ap.parse_args()
    voc = pkg.create_griffin_lim(seed=3)
    voc.set_opts(output_normalise=0)
    if not a.timing_only:
        accuracy(voc)
        properties(voc)
    for F in (800, 40):
        timing(voc, F)


if __name__ == "__main__":
    main()
