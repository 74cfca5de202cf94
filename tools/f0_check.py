"""The pitch tracker and pitch targets through the product alone: the device time of the two kernels
(k_f0_frames, k_f0_track; HIP events through xdtts_griffinlim_f0_linear_batch) at F = 800 and for 32 x F = 25, beside the
pitch branch of k_prosody / k_prosody_batch on the same magnitudes in the same run; the accuracy of tracker and targets on
synthetic voiced sounds (140 / 220 Hz, 3 % and 8 % vibrato; the true STFT magnitude and the same through the mel basis), all
through the device; the voicing strengths of voiced sound and of white noise; and the end-to-end distance between the median of
the GPU's audio and that of the fp32 CPU oracle chain (tests/test_gpu_f0.py holds its bound to twice this figure).

  python tools/f0_check.py                    # prints the table
  python tools/f0_check.py > profiles/f0.txt
"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import f0_ref as fr  # the restatement of the tests: measuring helpers only
import gpu_f0_cases as gc
import prosody_ref as pr


def best_median(call, key, n=20):
    call()  # warm: buffers, code object
    t = []
    for _ in range(n):
        call()
        t.append(voc.last_timings()[key] * 1e3)
    return min(t), float(np.median(t))


def timing():
    print("device time in us, best / median of 20 after a warm-up call (HIP events on the handle's stream):")
    for label, mags in (("F = 800", [pr.random_magnitude(800, seed=1)]), ("32 x F = 25", [pr.random_magnitude(25, seed=10 + u) for u in range(32)])):
        frames = best_median(lambda: voc.f0_linear_batch(mags), "mel_to_linear_ms")
        track = best_median(lambda: voc.f0_linear_batch(mags), "iterations_ms")
        pros = [pkg.Prosody(pitch=1.2)] * len(mags)
        if len(mags) == 1:
            prosody = best_median(lambda: voc.prosody_linear(mags[0], pros[0]), "mel_to_linear_ms")
        else:
            prosody = best_median(lambda: voc.prosody_linear_batch(mags, pros), "mel_to_linear_ms")
        print("  %-12s k_f0_frames %6.1f / %6.1f   k_f0_track %6.1f / %6.1f   k_prosody%s, pitch 1.2 (two transforms) %6.1f / %6.1f   frames / prosody %.2f"
              % (label, *frames, *track, "" if len(mags) == 1 else "_batch", *prosody, frames[1] / prosody[1]))
    big = [pr.random_magnitude(16384, seed=2)]
    o = pkg.F0Opts(threshold=0.0)
    print("  F = 16384, every frame voiced: k_f0_frames %.1f / %.1f   k_f0_track %.1f / %.1f"
          % (*best_median(lambda: voc.f0_linear_batch(big, opts=o), "mel_to_linear_ms", 10), *best_median(lambda: voc.f0_linear_batch(big, opts=o), "iterations_ms", 10)))


def accuracy():
    basis = np.asarray(pkg.create_mel_filter_bank(22050.0, 1024, 80, 0.0, 8000.0), dtype=np.float64)
    proj = np.linalg.pinv(basis) @ basis
    print("accuracy through the device, frames 4 .. F - 5 of F = 64, threshold 0.2 (cents against the instantaneous f0 (1 + v sin 2 pi 5 t)):")
    print("  f0   vibrato input  voiced  track max / rms   min strength   x0.85 median   x1.15 median   excursion in -> range 0 / range 2 (factor)")
    inner = slice(4, 60)
    for f0 in (140.0, 220.0):
        for vib in (0.03, 0.08):
            S_true = pr.stft_magnitude(pr.voiced_signal(n=256 * 63, f0=f0, vibrato=vib))
            for kind, S in (("true", S_true.astype(np.float32)), ("mel", np.maximum(proj @ S_true, 0.0).astype(np.float32))):
                raw, strength, est, st = voc.f0_linear(S)
                v = est > 0
                err = np.abs(fr.cents(est[inner][v[inner]], fr.true_f0(64, f0, vib)[inner][v[inner]]))
                med = []
                for k in (0.85, 1.15):
                    out, _, _ = voc.pitch_target_linear(S, pkg.PitchTarget(hz=k * f0))
                    e2 = voc.f0_linear(out)[2]
                    med.append(100.0 * (fr.lower_median(e2[inner][e2[inner] > 0]) / (k * f0) - 1.0))
                x = []
                for rng in (0.0, 2.0):
                    out, _, _ = voc.pitch_target_linear(S, pkg.PitchTarget(factor=1.0, range=rng))
                    e2 = voc.f0_linear(out)[2]
                    x.append(fr.excursion_cents(e2, e2 > 0))
                e_in = fr.excursion_cents(est, v)
                print("  %3.0f  %4.0f %%  %-5s  %5.3f   %5.1f / %4.1f       %.3f       %+6.2f %%       %+6.2f %%        %5.1f -> %5.1f / %5.1f (x %.2f)"
                      % (f0, 100 * vib, kind, v[inner].mean(), err.max(), np.sqrt(np.mean(err ** 2)), strength[inner].min(), med[0], med[1], e_in, x[0], x[1], x[1] / e_in))
    noise = 0.1 * np.random.default_rng(1).standard_normal(256 * 47)
    _, strength, _, st = voc.f0_audio(noise.astype(np.float32))
    print("white noise (0.1 x standard normal, 47 frames, through xdtts_griffinlim_f0_audio): largest strength %.3f, %d voiced at threshold 0.2" % (strength.max(), st.n_voiced))
    for f0 in (90.0, 70.0):
        S = np.maximum(proj @ pr.stft_magnitude(pr.voiced_signal(n=256 * 63, f0=f0, vibrato=0.03)), 0.0).astype(np.float32)
        _, strength, est, st = voc.f0_linear(S)
        print("the limit, through pinv(mel) . mel: a %g Hz voice: median strength %.3f, %d of 64 frames voiced, median %.1f Hz" % (f0, float(np.median(strength)), st.n_voiced, st.median_hz))


def end_to_end():
    import oracle

    r = gc.end_to_end(pkg, voc, oracle.Oracle("f32"), 160.0)
    print("end to end, 140 Hz voice -> log-mel -> infer_pitch_target(160 Hz), 30 iterations: source median %.2f Hz, base %.4f; median of the audio %.2f Hz,"
          " of the fp32 CPU oracle chain %.2f Hz, distance %.3f Hz (both by the fp64 restatement at threshold 0); xdtts_griffinlim_f0_audio on the audio at threshold 0: median %.2f Hz, median strength %.3f"
          % (r["stats"].median_hz, r["stats"].base_ratio, r["median_gpu"], r["median_cpu"], abs(r["median_gpu"] - r["median_cpu"]),
             r["stats_audio"].median_hz, r["strength_audio"]))


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("f0_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=30, seed=3)
    timing()
    accuracy()
    end_to_end()
