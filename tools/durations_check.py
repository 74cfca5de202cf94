"""The durations stage (per-id durations and timing marks from the cumulative attention) through the
product alone: per engine, the agreement of xdtts_tacotron2_last_durations with the fp64 oracle's cumulative weights after the
same steps (the cases of tests/test_gpu_durations.py: max, mean, the test's bound), the row sums, and the stage's cost -- the
headline utterance's xdtts_tacotron2_last_timings with the setting off and on, and the wall time of the call.

  python tools/durations_check.py                       # prints the table
  python tools/durations_check.py > profiles/durations.txt
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
wl = importlib.import_module("xd-tts_amd.workloads")
import oracle
import decoder_steps as ds
import durations_ref as dr
from durations_ref import BOUND, EXPECT_ENGINE, MAX_STEPS


def agreement():
    orc, orc64 = oracle.Oracle("f32"), oracle.Oracle("f64")
    blob = orc.weights_synthetic(seed=20240327, rec_scale=1.0)
    print("last_durations against the fp64 oracle's attention_weights_cum after the same steps, per id, in frames (bound %.1e):" % BOUND)
    print("  %-14s %-11s %2s | %10s %10s | %s" % ("case", "engine", "B", "max", "mean", "worst row sum |sum(dur) - F| / F"))
    for name, form, steps in dr.ENGINE_CASES:
        B, lens = len(steps), dr.case_lens(len(steps))
        with ds.form_env(form):
            m = pkg.Tacotron2.from_blob(blob)
            m.set_durations(on=1)
            m.infer_batch([dr.case_ids(n, b) for b, n in enumerate(lens)], fixed_steps=np.asarray(steps, dtype=np.int32),
                          opts=pkg.default_opts(dropout_seed=dr.DROPOUT_SEED, max_steps=MAX_STEPS, max_chunk=dr.WINDOW))
        errs, rows = [], []
        for b in range(B):
            dur = m.last_durations(b)[0].astype(np.float64)
            errs.append(np.abs(dur - dr.oracle_cum(orc64, blob, lens[b], b, steps[b])[0][:lens[b]]))
            rows.append(abs(dur.sum() - steps[b]) / steps[b])
        m.close()
        e = np.concatenate(errs)
        print("  %-14s %-11s %2d | %10.3e %10.3e | %.2e  %s" % (name, EXPECT_ENGINE[name], B, e.max(), e.mean(), max(rows), "ok" if e.max() <= BOUND else "OVER"))


def cost(n=8):
    model = pkg.Tacotron2.synthetic(seed=wl.WEIGHT_SEED, rec_scale=1.0)
    _ids, chunks, _steps = wl.config2(pkg)
    sp = np.cumsum([len(c) for c in chunks]).astype(np.int64)
    opts = pkg.default_opts(fixed_frames_per_id=wl.FRAMES_PER_ID, dropout_seed=0, item_base=0)
    ids = wl.synth_ids(120, seed=1)
    print("the headline utterance through xdtts_tacotron2_infer_ids, best of %d (last_timings: HIP events on the handle's stream; wall: the call):" % n)
    mels = {}
    for on in (0, 1, 0, 1):
        model.set_durations(on=on)
        model.infer(ids, splits=sp, opts=opts)  # warm: buffers
        best, wall = None, 1e30
        for _ in range(n):
            t0 = time.perf_counter()
            mels[on] = model.infer(ids, splits=sp, opts=opts)
            wall = min(wall, (time.perf_counter() - t0) * 1e3)
            t = model.last_timings()
            best = t if best is None or t["total_ms"] < best["total_ms"] else best
        print("  setting %-3s  encoder %.3f  decoder %.3f  postnet %.3f  total %.3f ms | wall %.3f ms | utterances captured %d" % (
            "on" if on else "off", best["encoder_ms"], best["decoder_ms"], best["postnet_ms"], best["total_ms"], wall, model.last_durations_count()))
    print("  mel with the setting on against off: %s" % ("bit for bit" if np.array_equal(mels[0], mels[1]) else "DIFFER"))
    s = model.last_alignment(0)
    print("  stats of the utterance: %s" % ", ".join("%s %d" % (f, getattr(s, f)) for f in dr.STATS_FIELDS))
    model.close()


if __name__ == "__main__":
    agreement()
    cost()
