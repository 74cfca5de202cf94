"""The output-rate stage (22 050 Hz -> 8 .. 96 kHz behind the loop) through the product alone:
the device time of k_resample on the headline utterance's 204 544 samples at 8000, 16000 and 48000 Hz (HIP events through the
parity hook), next to its traffic floor -- (N + N') 4 B plus the tap table once, over the achievable HBM rate -- and next to a
one-sample launch of the same kernel on the same stream (what a launch costs between two events); the worst |y - y_fp64| over
the a-priori bound for the shapes the GPU tests run; and `synthesize` of the headline utterance at 48000 against 22050.

  python tools/resample_check.py                       # prints the table
  python tools/resample_check.py > profiles/resample.txt
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
wl = importlib.import_module("xd-tts_amd.workloads")
import resample_ref as rr  # the fp64 restatement of the tests

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak
N_HEADLINE = 204544


def table_bytes(Q):
    """[L][T4] floats: the phase-major table the kernel reads (resample_plan.h)."""
    p = pkg.resample_plan(Q)
    L, H = p["L"], p["half_len"]
    T = H // L + (H + L - 1) // L + 1
    return L * ((T + 3) // 4 * 4) * 4


def stage_us(voc, x, Q, n=20):
    """Best and median of n: the stage alone (HIP events around the one launch on the handle's stream)."""
    voc.resample(x, Q)  # warm: table, buffers, code object
    us = []
    for _ in range(n):
        voc.resample(x, Q)
        us.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(us), float(np.median(us))


def timing(voc):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.0, 1.0, N_HEADLINE).astype(np.float32)
    print("device time of k_resample on N = %d samples (best / median of 20, HIP events on the handle's stream):" % N_HEADLINE)
    rows = {}
    for Q in (8000, 16000, 48000):
        p = pkg.resample_plan(Q, N_HEADLINE)
        tb = table_bytes(Q)
        floor = ((N_HEADLINE + p["n_out"]) * 4 + tb) / HBM_BYTES_PER_S * 1e6
        best, med = stage_us(voc, x, Q)
        empty, empty_med = stage_us(voc, x[:1], Q)
        taps = -(-(2 * p["half_len"] + 1) // p["L"])
        rows[Q] = best
        print("  rate %5d  L %3d / M %3d  N' = %6d  %3d taps per output, table %6.1f kB:  %6.1f us (median %6.1f)   traffic floor %5.2f us   one-sample launch %5.1f us (median %5.1f)   %.1f x the larger"
              % (Q, p["L"], p["M"], p["n_out"], taps, tb / 1e3, best, med, floor, empty, empty_med, best / max(floor, empty)))
        print("              %.1f G fused multiply-adds/s over the row entries, %.2f GB/s of input + output"
              % (p["n_out"] * (tb / 4 / p["L"]) / best * 1e-3, (N_HEADLINE + p["n_out"]) * 4 / best * 1e-3))
    return rows


def accuracy(voc):
    print("worst |y - y_fp64| / ((c + 2) 2^-24 sum |h||x|) through the hook, uniform noise and all ones, N in {1, 2, 255, 256, 257, 885, 4097, 9216}:")
    for Q in (8000, 11025, 44100, 48000, 32000):
        h = pkg.resample_filter(Q).astype(np.float64)
        rng = np.random.Generator(np.random.PCG64(1000 + Q))
        worst = 0.0
        for N in (1, 2, 255, 256, 257, 885, 4097, 9216):
            for x in (rng.uniform(-1.0, 1.0, N).astype(np.float32), np.ones(N, np.float32)):
                ref, c, a = rr.convolve(x, h, Q)
                worst = max(worst, float(np.max(np.abs(voc.resample(x, Q).astype(np.float64) - ref) / rr.bound(c, a))))
        print("  rate %5d: %.4f" % (Q, worst))


def filters():
    print("the library's own fp32 taps (numpy FFT): passband ripple up to 0.8 of the lower Nyquist, stopband from 1.0, phase DC gain:")
    for Q in rr.RATES:
        h = pkg.resample_filter(Q).astype(np.float64)
        p = rr.plan(Q)
        L, W = p["L"], max(p["L"], p["M"])
        nfft = 1 << 21
        db = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(h, nfft)) / L, 1e-300))
        f = np.arange(db.size) / nfft * 2.0 * W
        dc = max(abs(h[r::L].sum() - 1.0) for r in range(L))
        print("  rate %5d: %5d taps, ripple %.6f dB, stopband %.2f dB, DC within %.2e of 1" % (Q, h.size, np.max(np.abs(db[f <= 0.8])), np.max(db[f >= 1.0]), dc))


def headline(stage):
    model = pkg.Tacotron2.synthetic(seed=wl.WEIGHT_SEED, rec_scale=1.0)
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    _ids, chunks, _steps = wl.config2(pkg)
    sp = np.cumsum([len(c) for c in chunks]).astype(np.int64)
    opts = pkg.default_opts(fixed_frames_per_id=wl.FRAMES_PER_ID, dropout_seed=0, item_base=0)
    print("synthesize of the headline utterance (120 ids -> 800 frames, 60 iterations), 12 calls per rate after 3 warm-up calls, alternating blocks:")
    res = {22050: [], 48000: []}
    gl = {22050: [], 48000: []}
    for rep in range(3):
        for Q in (22050, 48000):
            voc.set_output_rate(Q)
            for g in range(5):
                t0 = time.perf_counter()
                _mel, audio = pkg.synthesize(model, voc, wl.synth_ids(120, seed=1 + g), splits=sp, opts=opts)
                dt = (time.perf_counter() - t0) * 1e3
                if g >= 1:
                    res[Q].append(dt)
                    gl[Q].append(voc.last_timings()["iterations_ms"])
            assert audio.size == pkg.resample_plan(Q, N_HEADLINE)["n_out"]
    for Q in (22050, 48000):
        print("  rate %5d: wall %.3f ms median (%.3f .. %.3f), vocoder ms[1] (loop + delivery stages) %.4f ms median" % (Q, np.median(res[Q]), min(res[Q]), max(res[Q]), np.median(gl[Q])))
    print("  difference: wall %+.1f us, vocoder ms[1] %+.1f us; the stage alone at 48000: %.1f us (its output is 2.18 x the samples: a longer copy to the host rides in the wall time)"
          % ((np.median(res[48000]) - np.median(res[22050])) * 1e3, (np.median(gl[48000]) - np.median(gl[22050])) * 1e3, stage[48000]))


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("resample_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    filters()
    rows = timing(voc)
    accuracy(voc)
    headline(rows)
