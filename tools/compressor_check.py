"""The dynamic range compressor through the product alone: the device time of the stage alone
(k_comp_init + k_comp_tiles + k_compress, HIP events through xdtts_griffinlim_compress) on the headline utterance's 204 544
samples at 22050 and on its N' samples at 8000 and 48000 under preset 1 ("drc") with the tests' speech-like signal; an all-zero
utterance (not engaged: pass 1 and the early exit of pass 2); a setting under which no sample is compressed (threshold 0 dB, hard
knee: every tile scans, r = 0 everywhere); a one-sample call; the traffic floor -- one read and one write of the signal over
the achievable HBM rate; then `infer` of the headline mel with rms normalisation, the stage off against preset 1; and what the
definition delivers on speech_like -- the spread between the 10th and 95th percentile of 400 ms block levels in front of and
behind preset 1, on the fp64 restatement (reported, not asserted) -- with the worst ratio of xdtts_compressor_reference to its
a-priori bound over the CPU tests' cases.

  python tools/compressor_check.py                       # prints the table
  python tools/compressor_check.py > profiles/compressor.txt
"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
import compressor_ref as cr  # the fp64 / integer restatement of the tests
import loudness_ref as lr

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak
N_HEADLINE = 204544


def stage_us(voc, x, Q, comp, n=20):
    """Best and median of n: the three launches alone (HIP events on the handle's stream); the stats of the last call."""
    voc.compress(x, Q, comp)  # warm: buffers, code object
    t = []
    for _ in range(n):
        _, st = voc.compress(x, Q, comp)
        t.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(t), float(np.median(t)), st


def timing(voc):
    drc = pkg.compressor_preset(1)
    flat = pkg.Compressor(threshold_db=0.0, ratio=3.0, knee_db=0.0)
    print("device time of the stage alone (k_comp_init + k_comp_tiles + k_compress; best / median of 20, HIP events):")
    for Q in (22050, 8000, 48000):
        n = pkg.resample_plan(Q, N_HEADLINE)["n_out"]
        x = lr.speech_like(Q, n, seed=3)
        p = pkg.compressor_plan(Q, drc)
        floor = 2 * n * 4 / HBM_BYTES_PER_S * 1e6
        print("  rate %5d  N = %6d (%3d tiles of 4096)   traffic floor (1 read + 1 write) %5.2f us   alpha %d rho %d" % (Q, n, -(-n // 4096), floor, p["alpha"], p["rho"]))
        best, med, st = stage_us(voc, x, Q, drc)
        assert st.engaged == 1 and st.compressed > 0
        print("    preset 1 (drc):            %6.1f us (median %6.1f; %6d samples compressed, max_over %d)" % (best, med, st.compressed, st.max_over))
        best, med, st = stage_us(voc, x, Q, flat)
        assert st.engaged == 1 and st.compressed == 0
        print("    nothing over the threshold: %6.1f us (median %6.1f)" % (best, med))
        best, med, st = stage_us(voc, np.zeros(n, dtype=np.float32), Q, drc)
        assert st.engaged == 0
        print("    all zero, not engaged:      %6.1f us (median %6.1f)" % (best, med))
        best, med, _ = stage_us(voc, x[:1], Q, drc)
        print("    a one-sample call           %6.1f us (median %6.1f)" % (best, med))


def delivered():
    """infer of an 800-frame mel, 60 iterations: ms[1] = the loop and the delivery stages."""
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    rng = np.random.default_rng(4)
    mel = (rng.uniform(-7.0, -1.0, size=(80, 800)) + 1.5 * np.sin(np.arange(800) / 4.0)[None, :]).astype(np.float32)
    print("infer of an 800-frame mel (60 iterations, rms normalisation), vocoder ms[1] = loop + delivery stages, median of 15 after 3 warm-up calls, alternating:")
    forms = (("compressor off", None), ("preset 1 (drc)", pkg.compressor_preset(1)))
    for Q in (22050, 8000):
        voc.set_output_rate(Q)
        ms = {f[0]: [] for f in forms}
        info = {}
        for rep in range(18):
            for name, comp in forms:
                voc.set_compressor(comp)
                voc.infer(mel)
                if rep >= 3:
                    ms[name].append(voc.last_timings()["iterations_ms"])
                info[name] = voc.last_compressor()
        base = float(np.median(ms[forms[0][0]]))
        for name, _ in forms:
            st = info[name]
            tail = "   engaged %d, %d samples compressed" % (st[0].engaged, st[0].compressed) if st else ""
            print("  rate %5d  %-16s %.4f ms  (%+.1f us)%s" % (Q, name, np.median(ms[name]), (np.median(ms[name]) - base) * 1e3, tail))
    voc.close()


def effect():
    print("what the definition delivers on speech_like (fp64 restatement; reported, not asserted):")
    for Q in (22050, 8000):
        x = lr.speech_like(Q, 10 * Q, seed=3)
        ref = cr.compress(x, Q, cr.settings(**cr.DRC))
        a, b = cr.block_level_spread(x, Q), cr.block_level_spread(ref["out"], Q)
        print("  rate %5d, 10 s: spread of the 400 ms block levels, 95th - 10th percentile: %.2f dB in front, %.2f dB behind preset 1 (%d of %d samples compressed)"
              % (Q, a, b, ref["compressed"], x.size))
    worst = 0.0
    for Q in cr.RATES:
        for kind in cr.KINDS:
            x = cr.signal(kind, Q, 2 * cr.TILE + 301)
            for kw in (cr.DRC, dict(cr.DRC, ratio=20.0, knee_db=0.0, attack_ms=0.1, release_ms=1.0), dict(cr.DRC, ratio=1.5, knee_db=24.0, attack_ms=100.0, release_ms=2000.0),
                       dict(cr.DRC, makeup_db=6.0)):
                c = cr.settings(**kw)
                out, _ = pkg.compressor_reference(x, Q, pkg.Compressor(**kw))
                ref = cr.compress(x, Q, c)
                lim = np.abs(ref["out"]) * cr.gain_bound(Q, c)
                err = np.abs(out - ref["out"])
                worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print("xdtts_compressor_reference against the fp64 restatement, the CPU tests' 60 cases: worst |out - out64| / a-priori bound = %.4f" % worst)


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("compressor_check.py needs a HIP device: nothing here is measured without one")
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    timing(voc)
    delivered()
    effect()
