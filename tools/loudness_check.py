"""The loudness stage (BS.1770 integrated loudness under a true-peak ceiling behind the resampler)
through the product alone: the device time of the four measuring launches on the headline utterance's 204 544 samples at 22050
and on its N' samples at 8000 and 48000 (HIP events through the measurement hook), next to the traffic floor -- three reads and
one write of the signal over the achievable HBM rate -- and next to a one-sample call of the same kernels; the same with the
recurrences in fp32 (XDTTS_LOUD=fp32) and what that does to the reading; `infer` of the headline mel with a target on against
output_normalise 0 and 3 (the stage with its scaling launch, inside ms[1]); the worst error ratios of the hook tests.

  python tools/loudness_check.py                       # prints the table
  python tools/loudness_check.py > profiles/loudness.txt
"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import loudness_ref as lr  # the fp64 restatement of the tests

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak
N_HEADLINE = 204544


def stage_us(voc, x, Q, n=20):
    """Best and median of n: the four measuring launches alone (HIP events on the handle's stream)."""
    voc.loudness(x, Q)  # warm: table, buffers, code object
    us = []
    for _ in range(n):
        voc.loudness(x, Q)
        us.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(us), float(np.median(us))


def timing(voc):
    print("device time of the measurement (k_loud_local, k_loud_carry, k_loud_energy, k_loud_final; best / median of 20, HIP events):")
    for Q in (22050, 8000, 48000):
        n = pkg.resample_plan(Q, N_HEADLINE)["n_out"]
        x = lr.speech_like(Q, n, seed=3)
        floor = 4 * n * 4 / HBM_BYTES_PER_S * 1e6  # measurement 2 reads, scaling 1 read + 1 write
        best, med = stage_us(voc, x, Q)
        one, one_med = stage_us(voc, x[:1], Q)
        os.environ["XDTTS_LOUD"] = "fp32"
        try:
            b32, m32 = stage_us(voc, x, Q)
        finally:
            del os.environ["XDTTS_LOUD"]
        print("  rate %5d  N = %6d (%3d groups of 2048, %5d segments of 32):  fp64 %6.1f us (median %6.1f)   fp32 recurrences %6.1f us (median %6.1f)"
              "   traffic floor (3 reads + 1 write) %5.2f us   one-sample call %5.1f us (median %5.1f)"
              % (Q, n, -(-n // 2048), -(-n // 32), best, med, b32, m32, floor, one, one_med))


def fp32_error(voc):
    print("what the fp32 recurrences do to the reading (1.5 s of the tests' signal; |L - L_fp64| in LU, gated blocks device / fp64):")
    for Q in (22050, 48000, 96000):
        x = lr.speech_like(Q, int(1.5 * Q), seed=5)
        m = lr.measure(x, Q)
        d64 = voc.loudness(x, Q)
        os.environ["XDTTS_LOUD"] = "fp32"
        try:
            d32 = voc.loudness(x, Q)
        finally:
            del os.environ["XDTTS_LOUD"]
        print("  rate %5d: fp64 %.2e LU (%d / %d)   fp32 %.2e LU (%d / %d)"
              % (Q, abs(d64.lufs - m["lufs"]), d64.gated_blocks, m["gated_blocks"], abs(d32.lufs - m["lufs"]), d32.gated_blocks, m["gated_blocks"]))


def accuracy(voc):
    print("the hook tests' shapes: worst |Z - Z_fp64| / (1e-7 Z) and worst |TP - TP_fp64| / (26 2^-24 sum |t||x|) per rate:")
    taps = pkg.true_peak_filter().astype(np.float64)
    for Q in lr.GPU_RATES:
        w_ms = w_tp = 0.0
        for N in lr.lengths(Q):
            x = lr.speech_like(Q, N)
            m, d = lr.measure(x, Q), voc.loudness(x, Q)
            assert (d.blocks, d.gated_blocks) == (m["blocks"], m["gated_blocks"])
            if m["mean_square"] > 0:
                w_ms = max(w_ms, abs(d.mean_square - m["mean_square"]) / m["mean_square"] / 1e-7)
            tp, _, bound = lr.true_peak(x, taps)
            w_tp = max(w_tp, abs(d.true_peak - tp) / bound)
        print("  rate %5d: %.5f   %.4f" % (Q, w_ms, w_tp))


def delivered():
    """infer of an 800-frame mel, 60 iterations: ms[1] = the loop and the delivery stages."""
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    rng = np.random.default_rng(4)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 800)) + 1.5 * np.sin(np.arange(800) / 4.0)[None, :]).astype(np.float32)
    print("infer of an 800-frame mel (60 iterations), vocoder ms[1] = loop + delivery stages, median of 15 after 3 warm-up calls, alternating:")
    forms = (("output_normalise 0", 0, None), ("output_normalise 3", 3, None), ("target -16 LUFS, ceiling -1 dBTP", 3, -16.0))
    for Q in (22050, 48000):
        voc.set_output_rate(Q)
        ms = {name: [] for name, _, _ in forms}
        for rep in range(18):
            for name, mode, target in forms:
                voc.set_opts(output_normalise=mode)
                voc.set_loudness(target, -1.0 if target is not None else None)
                voc.infer(mel)
                if rep >= 3:
                    ms[name].append(voc.last_timings()["iterations_ms"])
        base = float(np.median(ms[forms[0][0]]))
        for name, _, _ in forms:
            print("  rate %5d  %-34s %.4f ms  (%+.1f us)" % (Q, name, np.median(ms[name]), (np.median(ms[name]) - base) * 1e3))
        (l,) = voc.last_loudness()
        print("              last_loudness: %.3f LUFS measured, gain %.4f, true peak %.4f -> %.4f, %d of %d blocks gated"
              % (l.lufs, l.gain, l.true_peak, l.gain * l.true_peak, l.gated_blocks, l.blocks))
    voc.close()


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("loudness_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    timing(voc)
    fp32_error(voc)
    accuracy(voc)
    delivered()
