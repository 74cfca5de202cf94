"""Developer aid (python tools/pair_step.py NAME; profiles/pair_step.txt): us per step of the gate-less pair (two 95-id chunks), the gate-on pair and the one-chunk kernel for the
library named by XDTTS_LIB; slope between 200 and 600 steps (set-up cancels), best of 5 each; and a hash of the mels."""
import hashlib, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("xd-tts_amd")
synth_ids = importlib.import_module("xd-tts_amd.workloads").synth_ids
name = sys.argv[1]
m = pkg.Tacotron2.synthetic()
h = hashlib.sha256()


def best(ids, n, reps=5, **kw):
    b = 1e9
    for _ in range(reps):
        mels = m.infer_batch(ids, opts=pkg.default_opts(dropout_seed=1, **kw.get("o", {})), **kw.get("k", {}))
        b = min(b, m.last_timings()["decoder_ms"] * 1e3)
    for x in mels:
        h.update(np.ascontiguousarray(x, dtype=np.float32).tobytes())
    return b


pair = [synth_ids(95, seed=1), synth_ids(95, seed=2)]
res = {}
for tag, ids, mk in (("pair", pair, lambda n: dict(k=dict(fixed_steps=[n, n]))),
                     ("pair_gate", pair, lambda n: dict(o=dict(max_steps=n))),
                     ("one", pair[:1], lambda n: dict(k=dict(fixed_steps=[n])))):
    t2, t6 = best(ids, 200, **mk(200)), best(ids, 600, **mk(600))
    res[tag] = ((t6 - t2) / 400.0, t6 / 600.0)
# the headline's shape: 95 + 25 ids, 633 / 167 frames (pair launch of 167 steps, then the survivor alone)
hl = best([synth_ids(95, seed=1), synth_ids(25, seed=2)], 0, k=dict(fixed_steps=[633, 167]))
print("%-10s pair %.3f (%.3f)  pair_gate %.3f (%.3f)  one %.3f (%.3f) us/step slope (t600/600)  headline-shape loop %.1f us  mels %s"
      % (name, res["pair"][0], res["pair"][1], res["pair_gate"][0], res["pair_gate"][1], res["one"][0], res["one"][1], hl, h.hexdigest()[:16]),
      "engine", m.engine_state()["decoder_persistent"], flush=True)
