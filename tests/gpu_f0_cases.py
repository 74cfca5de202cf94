"""The magnitudes the pitch-tracker tests share (tests/test_f0_cpu.py checks on the CPU what tests/test_gpu_f0.py relies on)."""
import numpy as np

import prosody_ref as pr

FRAMES = [1, 2, 5, 37, 64]


def voiced_magnitudes(pkg):
    """{(f0, kind): S (513, 64) float32}: voiced_signal(256 * 63, f0, vibrato 0.03) at 140 and 220 Hz -- its true STFT magnitude
    ("true"), and the same through pinv(mel_basis) . mel_basis ("mel"), what mel -> linear can return of it."""
    basis = np.asarray(pkg.create_mel_filter_bank(22050.0, 1024, 80, 0.0, 8000.0), dtype=np.float64)
    proj = np.linalg.pinv(basis) @ basis
    out = {}
    for f0 in (140.0, 220.0):
        S = pr.stft_magnitude(pr.voiced_signal(n=256 * 63, f0=f0, vibrato=0.03))
        out[(f0, "true")] = S.astype(np.float32)
        out[(f0, "mel")] = np.maximum(proj @ S, 0.0).astype(np.float32)
    return out


def frame_cases(voiced):
    """{name: S (513, F)} of the per-frame parity test: random magnitudes with 5 % exact zeros at every F, the four voiced
    magnitudes, an all-zero one."""
    out = {"random%d" % F: pr.random_magnitude(F, seed=100 + F) for F in FRAMES}
    for (f0, kind), S in voiced.items():
        out["voiced%d%s" % (int(f0), kind)] = S
    out["zero37"] = np.zeros((513, 37), dtype=np.float32)
    return out


def end_to_end(pkg, voc, orc, hz=160.0):
    """The end-to-end chain of tests/test_gpu_f0.py and tools/f0_check.py: the log-mel of the 140 Hz voice (the GPU's own analysis)
    -> infer_pitch_target at `hz` (the handle's iterations), and beside it the fp32 CPU oracle chain given the device's own ratios
    (the oracle's mel -> linear, the float32 restatement of the stage, the oracle's Griffin-Lim from its seeded phase).  Both
    medians are estimated by f0_ref (fp64) on the audio's fp64 STFT magnitude, frames 4 .. F - 5, at threshold 0: the signal is
    voiced throughout, so no voicing decision is wanted -- and Griffin-Lim audio from a mel carries a cepstral peak of only about
    0.15 (0.12 without a target; the source signal has 0.4), under the default threshold.  Returns a dict."""
    import f0_ref as fr

    y = pr.voiced_signal(n=256 * 63, f0=140.0, vibrato=0.03)
    _, mel = voc.analyze(y, want_S=False)
    t = pkg.PitchTarget(hz=hz)
    audio = voc.infer_pitch_target(mel, t)
    stats = voc.last_f0()[0]
    _, ratio, stats_hook = voc.pitch_target_linear(voc.mel_to_linear(mel), t)
    _, strength_audio, _, stats_audio = voc.f0_audio(audio, opts=pkg.F0Opts(threshold=0.0))
    S_cpu = orc.mel_to_linear(orc.pinv(orc.mel_filter_bank()), mel, power=1.7)
    c, one, gain = fr.rate1_table(64)
    S_mod = fr.apply_table(S_cpu, c, fr.table_pitch(one, ratio), gain, dtype=np.float32)
    audio_cpu = orc.griffinlim(S_mod, phase0=orc.phase_init(3, 513, 64), iters=30)

    def median_of(a):
        o = fr.opts(threshold=0.0)
        _, raw, strength, _ = fr.frames(pr.stft_magnitude(a).astype(np.float32), o, np.float64)
        f0, v, _, _ = fr.track(raw.astype(np.float32), strength.astype(np.float32), o)
        return float(fr.lower_median(f0[4:-4][v[4:-4]]))

    return dict(stats=stats, stats_hook=stats_hook, stats_audio=stats_audio, strength_audio=float(np.median(strength_audio)), median_gpu=median_of(audio), median_cpu=median_of(audio_cpu))
