"""The silence stage through the product alone: the device time of the stage alone (k_sil_peaks +
k_sil_plan + k_sil_gather, HIP events through xdtts_griffinlim_trim) on the headline utterance's 204 544 samples at 22050 and on
its N' samples at 48000, with the tests' speech-like signal under the defaults and with a pause cap, an all-zero utterance and a
one-sample call, beside the traffic floor -- one read and one write of the signal over the achievable HBM rate; then `infer` of
the headline mel with the stage off against the stage on: its share of the vocoder half, next to the compressor's figure from
profiles/compressor.txt.  Measured, not asserted.

  python tools/silence_check.py                       # prints the table
  python tools/silence_check.py > profiles/silence.txt
"""
import importlib, os, re, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import loudness_ref as lr

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak
N_HEADLINE = 204544
RATES = (22050, 48000)


def stage_us(voc, x, Q, sil, n=20):
    """Best and median of n: the three launches alone (HIP events on the handle's stream); the stats of the last call."""
    voc.trim(x, Q, sil)  # warm: buffers, code object
    t = []
    for _ in range(n):
        _, st = voc.trim(x, Q, sil)
        t.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(t), float(np.median(t)), st


def timing(voc):
    print("device time of the stage alone (k_sil_peaks + k_sil_plan + k_sil_gather; best / median of 20, HIP events):")
    for Q in RATES:
        n = pkg.resample_plan(Q, N_HEADLINE)["n_out"]
        x = lr.speech_like(Q, n, seed=3)
        p = pkg.silence_plan(Q, pkg.Silence())
        floor = 2 * n * 4 / HBM_BYTES_PER_S * 1e6
        print("  rate %5d  N = %6d (%3d tiles of 4096, %4d windows of %d)   traffic floor (1 read + 1 write) %5.2f us" %
              (Q, n, -(-n // 4096), -(-n // p["W"]), p["W"], floor))
        for name, sil in (("the defaults", pkg.Silence()), ("threshold -30, pauses <= 100 ms", pkg.Silence(threshold_db=-30.0, max_pause_ms=100.0))):
            best, med, st = stage_us(voc, x, Q, sil)
            print("    %-32s %6.1f us (median %6.1f; n_out %6d, cut lead %d trail %d pause %d, %d cuts)" %
                  (name + ":", best, med, st.n_out, st.lead_cut, st.trail_cut, st.pause_cut, st.n_cuts))
        best, med, st = stage_us(voc, np.zeros(n, dtype=np.float32), Q, pkg.Silence())
        assert st.any_sound == 0
        print("    %-32s %6.1f us (median %6.1f; n_out %d)" % ("all zero, no sound:", best, med, st.n_out))
        best, med, _ = stage_us(voc, x[:1] + np.float32(0.1), Q, pkg.Silence())
        print("    %-32s %6.1f us (median %6.1f)" % ("a one-sample call:", best, med))


def delivered():
    """infer of an 800-frame mel, 60 iterations: ms[2] = the vocoder half, ms[1] = the loop and the delivery stages."""
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    rng = np.random.default_rng(4)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 800)) + 1.5 * np.sin(np.arange(800) / 4.0)[None, :]).astype(np.float32)
    print("infer of an 800-frame mel (60 iterations, rms normalisation), median of 15 after 3 warm-up calls, alternating; ms[1] = loop + delivery stages, ms[2] = the vocoder half:")
    forms = (("silence off", None), ("the defaults", pkg.Silence()))
    shares = {}
    for Q in RATES:
        voc.set_output_rate(Q)
        ms = {f[0]: ([], []) for f in forms}
        info = {}
        for rep in range(18):
            for name, sil in forms:
                voc.set_silence(sil)
                voc.infer(mel)
                if rep >= 3:
                    t = voc.last_timings()
                    ms[name][0].append(t["iterations_ms"])
                    ms[name][1].append(t["total_ms"])
                info[name] = voc.last_silence()
        base = float(np.median(ms[forms[0][0]][0]))
        for name, _ in forms:
            st = info[name]
            tail = "   n_out %d of %d, %d cuts" % (st[0].n_out, st[0].n_in, st[0].n_cuts) if st else ""
            add = (float(np.median(ms[name][0])) - base) * 1e3
            print("  rate %5d  %-14s ms[1] %.4f ms  (%+.1f us)   ms[2] %.4f ms%s" % (Q, name, np.median(ms[name][0]), add, np.median(ms[name][1]), tail))
        shares[Q] = 100.0 * (float(np.median(ms[forms[1][0]][0])) - base) / (1e-9 + float(np.median(ms[forms[1][0]][1])))
        print("  rate %5d  the stage's share of the vocoder half: %.1f %%" % (Q, shares[Q]))
    voc.close()


def beside_the_compressor():
    path = os.path.join(ROOT, "profiles", "compressor.txt")
    if not os.path.exists(path):
        return
    text = open(path).read()
    print("the compressor's figures (profiles/compressor.txt), for comparison:")
    for line in text.splitlines():
        if re.search(r"preset 1 \(drc\)", line):
            print("  " + line.strip())


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("silence_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    timing(voc)
    delivered()
    beside_the_compressor()
