"""The look-ahead true-peak limiter through the product alone: the device time of the stage alone
(k_limit_init + k_limit, HIP events through xdtts_griffinlim_limit) on the headline utterance's 204 544 samples at 22050 and on
its N' samples at 8000 and 48000, at 500 / 5000 / 10000 us of look-ahead, with the tests' speech-like signal driven over a
-3 dBTP ceiling (engaged: the hold, the smoothing and its skipped rounds) and with a gain under which no sample needs limiting
(every tile stages, votes and scales); a one-sample call; the traffic floor -- one read and one write of the signal over the
achievable HBM rate; then `infer` of the headline mel with a target on: k_loud_scale (limiter off) against k_limit, where the
ceiling binds and where it does not (the scale route alone, no staging).

  python tools/limiter_check.py                       # prints the table
  python tools/limiter_check.py > profiles/limiter.txt
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
T_LUFS, C_LIN = -10.0, 10.0 ** (-3.0 / 20.0)


def stage_us(voc, x, Q, g0, us, n=20):
    """Best and median of n: the two launches alone (HIP events on the handle's stream); the stats of the last call."""
    voc.limit(x, Q, g0, C_LIN, us)  # warm: window, buffers, code object
    t = []
    for _ in range(n):
        _, st = voc.limit(x, Q, g0, C_LIN, us)
        t.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(t), float(np.median(t)), st


def timing(voc):
    print("device time of the stage alone (k_limit_init + k_limit; best / median of 20, HIP events), -10 LUFS under -3 dBTP:")
    for Q in (22050, 8000, 48000):
        n = pkg.resample_plan(Q, N_HEADLINE)["n_out"]
        x = lr.speech_like(Q, n, seed=3)
        m = lr.measure(x, Q)
        g0 = lr.gain(m["mean_square"], m["true_peak"], T_LUFS)
        assert g0 * m["true_peak"] > C_LIN
        quiet = 0.5 * C_LIN / m["true_peak"]
        floor = 2 * n * 4 / HBM_BYTES_PER_S * 1e6
        print("  rate %5d  N = %6d (%3d tiles of 4096)   traffic floor (1 read + 1 write) %5.2f us" % (Q, n, -(-n // 4096), floor))
        for us in (500, 5000, 10000):
            H = pkg.limiter_plan(Q, us)["half_width"]
            best, med, st = stage_us(voc, x, Q, g0, us)
            qb, qm, qst = stage_us(voc, x, Q, quiet, us)
            assert qst.limited == 0 and st.limited > 0
            print("    %5d us (H = %3d):  engaged %7.1f us (median %7.1f; %6d samples limited, min gain %.4f)   nothing over the ceiling %6.1f us (median %6.1f)"
                  % (us, H, best, med, st.limited, st.min_gain, qb, qm))
        one, one_med, _ = stage_us(voc, x[:1], Q, g0, 5000)
        print("    a one-sample call %5.1f us (median %5.1f)" % (one, one_med))


def delivered():
    """infer of an 800-frame mel, 60 iterations: ms[1] = the loop and the delivery stages."""
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    rng = np.random.default_rng(4)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 800)) + 1.5 * np.sin(np.arange(800) / 4.0)[None, :]).astype(np.float32)
    print("infer of an 800-frame mel (60 iterations), vocoder ms[1] = loop + delivery stages, median of 15 after 3 warm-up calls, alternating:")
    forms = (("-10 LUFS / -3 dBTP, k_loud_scale", -10.0, -3.0, 0), ("-10 LUFS / -3 dBTP, limiter 5 ms", -10.0, -3.0, 5000),
             ("-40 LUFS / +6 dBTP, k_loud_scale", -40.0, 6.0, 0), ("-40 LUFS / +6 dBTP, limiter 5 ms", -40.0, 6.0, 5000))
    for Q in (22050, 48000):
        voc.set_output_rate(Q)
        ms = {f[0]: [] for f in forms}
        info = {}
        for rep in range(18):
            for name, T, C, us in forms:
                voc.set_loudness(T, C)
                voc.set_limiter(us)
                y = voc.infer(mel)
                if rep >= 3:
                    ms[name].append(voc.last_timings()["iterations_ms"])
                if rep == 17:
                    info[name] = (lr.measure(y, Q)["lufs"], voc.last_limiter())
        base = float(np.median(ms[forms[0][0]]))
        for name, _, _, _ in forms:
            lufs, st = info[name]
            tail = "   engaged %d, %d samples limited, min gain %.4f" % (st[0].engaged, st[0].limited, st[0].min_gain) if st else ""
            print("  rate %5d  %-34s %.4f ms  (%+.1f us)   delivered %.2f LUFS%s" % (Q, name, np.median(ms[name]), (np.median(ms[name]) - base) * 1e3, lufs, tail))
    voc.close()


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("limiter_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    timing(voc)
    delivered()
