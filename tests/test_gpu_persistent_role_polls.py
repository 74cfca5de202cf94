"""The persistent decoder's role workgroups issue the first poll of the vector they gather next from inside the column block
behind their own publish (csrc/decoder_persistent.hip, EPOLL_AT / MPOLL_AT), and no publish is followed by a wait.
A poll that leaves too early, or a publish that moved, must only ever cost time:

  * one chunk (the one-chunk kernel) and two chunks of unequal length (the skewed pair, whose survivor continues on the one-chunk
    kernel; either chunk may be the survivor), 5 and 9 steps (the two granule slots of a value are reused every second step);
  * encoder windows T = 8, 64, 65 (the first step of the second lane half) and 100 (the engine's shape), a chunk as long as its window;
  * gate off (fixed frame counts) and gate on, rigged with xd-tts_amd/gate_rig.py to stop the chunks after exactly 9 and 5 frames.

Every shape is compared with the CPU oracle at the tolerance of test_gpu_decoder_paths.py (frames and mels 1e-5 RMS, gate logits
and alignments 1e-5 absolute), and must be bit-identical to the same request with one workgroup stalling ~7 us at a different
point of every step (XDTTS_PERSIST_SLOW, the hook of test_gpu_stragglers.py): an attention workgroup, a projection workgroup, a plain
LSTM slice.  No case loses a workgroup or runs into a time-out."""
import importlib

import numpy as np
import pytest

from conftest import rms, synth_ids
from test_gpu_stragglers import env

pytestmark = pytest.mark.gpu

WINDOWS = (8, 64, 65, 100)
STEPS = (9, 5)     # of chunk 0 and chunk 1; the rigged gate stops them there
SEED = 41
NAMES = {"attention_hidden": "att_h", "attention_cell": "att_c", "decoder_hidden": "dec_h", "decoder_cell": "dec_c",
         "attention_weights": "aw", "attention_weights_cum": "awc", "attention_context": "ctx"}


def slow_workgroups(B):
    """XDTTS_PERSIST_SLOW values (workgroup index + 1) of a B-chunk launch: attention role, projection + prenet role, plain slice."""
    return (1, 8 * B + 2, 201)


_CASES = {}


def case(pkg, model, orc, blob, T):
    """Per window, made once: two chunks (T and T // 2 + 1 ids), their oracle encodings, and the weights with the gate rigged to stop
    them after STEPS frames (gate_rig records the gate's inputs on the GPU at this window and solves for the gate layer)."""
    if T not in _CASES:
        rig = importlib.import_module("xd-tts_amd.gate_rig")
        ids = [synth_ids(T, seed=700 + T), synth_ids(T // 2 + 1, seed=800 + T)]
        enc = []
        for x in ids:
            padded = np.zeros(T, dtype=np.int64)
            padded[: len(x)] = x
            enc.append(orc.encoder(blob, padded))
        X = rig.record_gate_inputs(pkg, model, ids, list(STEPS), pkg.default_opts(dropout_seed=SEED), window=T)
        w, b, slack, _ = rig.solve_gate(X, list(STEPS))
        assert slack > 1e-3, slack   # (logits; the oracle's trajectory is within 1e-5 of the recorded one)
        rblob = np.array(blob, dtype=np.float32, copy=True)
        tab = {n: off for n, _shape, off in pkg.tensor_table()}
        rblob[tab["gate_layer.weight"] : tab["gate_layer.weight"] + 1536] = w.astype(np.float32)
        rblob[tab["gate_layer.bias"]] = np.float32(b)
        _CASES[T] = dict(ids=ids, enc=enc, rblob=rblob, handle=pkg.Tacotron2.from_blob(rblob))
    return _CASES[T]


@pytest.fixture(scope="module", autouse=True)
def _close_rigged_handles():
    yield
    for c in _CASES.values():
        c["handle"].close()
    _CASES.clear()


def with_stragglers(B, run):
    """run() undisturbed, then with each straggler: every array of the result bit-identical."""
    want = run()
    for wg in slow_workgroups(B):
        with env(XDTTS_PERSIST_SLOW=wg):
            got = run()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (wg, g.shape, w.shape)
    return want


@pytest.mark.parametrize("gate", ["off", "on"])
@pytest.mark.parametrize("T", WINDOWS)
def test_one_chunk_frames_gates_and_alignment(pkg, model, orc, blob, T, gate):
    """The one-chunk kernel from step 0: chunk 0 for 9 steps and chunk 1 (in its own dropout stream, item 1) for 5 -- by a fixed count,
    or stopped by the rigged gate.  Frames and gate logits of the decode entry, and the alignment (with the other six state
    tensors) that the parity hook returns after the same number of steps, against the oracle's."""
    c = case(pkg, model, orc, blob, T)
    m, wblob = (c["handle"], c["rblob"]) if gate == "on" else (model, blob)
    for b, n in enumerate(STEPS):
        mem, pm = c["enc"][b]
        nv = len(c["ids"][b])
        fixed = dict(fixed_steps=n) if gate == "off" else dict(max_steps=16)
        rframes, rgates = orc.run_decoder(wblob, mem, pm, nv, orc.default_opts(dropout_seed=SEED, item=b, **fixed))
        assert rframes.shape == (n, 80)   # (gate on: the oracle's own stop rule ends at the rigged frame)
        o = pkg.default_opts(dropout_seed=SEED, item_base=b, **fixed)
        frames, gates = with_stragglers(1, lambda: m.decoder(mem, pm, nv, o))
        assert frames.shape == rframes.shape, (frames.shape, rframes.shape)
        assert rms(frames, rframes) <= 1e-5 and np.abs(gates - rgates).max() <= 1e-5
        # the same steps through the parity hook: the state it writes back
        st = orc.new_state()
        oo = orc.default_opts(dropout_seed=SEED, item=b)
        for s in range(n):
            orc.decoder_step(wblob, mem, pm, nv, st, oo, s)
        zero = {"attention_hidden": 1024, "attention_cell": 1024, "decoder_hidden": 1024, "decoder_cell": 1024,
                "attention_weights": T, "attention_weights_cum": T, "attention_context": 512}
        z = {k: np.zeros((1, d), dtype=np.float32) for k, d in zero.items()}
        ho = pkg.default_opts(dropout_seed=SEED, item_base=b)

        def hook():
            out, gt, gst = m.decoder_steps("persistent", mem[None], pm[None], [nv], z, np.zeros((1, 80), dtype=np.float32), 0, n, ho)
            return [out, gt] + [gst[k] for k in NAMES]

        got = with_stragglers(1, hook)
        assert rms(got[0][0], rframes) <= 1e-5 and np.abs(got[1][0] - rgates).max() <= 1e-5
        for k, arr in zip(NAMES, got[2:]):
            ref = np.array(getattr(st, NAMES[k]), dtype=np.float32)[: arr.shape[1]]
            assert np.abs(arr[0] - ref).max() <= 1e-5, (k, T, b)
    assert m.engine_state()["decoder_persistent"] == 1   # no exchange timed out


@pytest.mark.parametrize("gate", ["off", "on"])
@pytest.mark.parametrize("T", WINDOWS)
def test_pair_hands_over_to_the_one_chunk_kernel(pkg, model, orc, blob, T, gate):
    """Two chunks of unequal length through the public batch entry: the skewed pair runs until the shorter sequence ends and the
    one-chunk kernel continues the survivor -- chunk 0 (9 and 5 frames) and, gate off, chunk 1 (5 and 9 frames).  Mels (post-net
    included) against the oracle's infer_chunk at this window."""
    c = case(pkg, model, orc, blob, T)
    m, wblob = (c["handle"], c["rblob"]) if gate == "on" else (model, blob)
    for steps in ((STEPS,) if gate == "on" else (STEPS, STEPS[::-1])):
        if gate == "on":
            o, kw = pkg.default_opts(dropout_seed=SEED, max_chunk=T, max_steps=16), {}
        else:
            o, kw = pkg.default_opts(dropout_seed=SEED, max_chunk=T), dict(fixed_steps=np.asarray(steps, dtype=np.int32))
        mels = with_stragglers(2, lambda: m.infer_batch(c["ids"], opts=o, **kw))
        for b, n in enumerate(steps):
            fixed = dict(fixed_steps=n) if gate == "off" else dict(max_steps=16)
            ref = orc.infer_chunk(wblob, c["ids"][b], orc.default_opts(dropout_seed=SEED, item=b, **fixed), window=T)
            assert mels[b].shape == ref.shape == (80, n), (mels[b].shape, ref.shape)
            assert rms(mels[b], ref) <= 1e-5, (T, b)
    assert m.engine_state()["decoder_persistent"] == 1


@pytest.mark.parametrize("T", WINDOWS)
def test_lock_step_pair_alignment(pkg, model, orc, blob, T):
    """The lock-step pair loop (the parity hook's form of a two-chunk launch; it shares the column blocks and the gather with the
    one-chunk kernel): both chunks 5 and 9 steps from step 0, frames, gate logits and the written-back state against the oracle."""
    c = case(pkg, model, orc, blob, T)
    mem = np.stack([e[0] for e in c["enc"]])
    pm = np.stack([e[1] for e in c["enc"]])
    nv = [len(x) for x in c["ids"]]
    dims = {"attention_hidden": 1024, "attention_cell": 1024, "decoder_hidden": 1024, "decoder_cell": 1024,
            "attention_weights": T, "attention_weights_cum": T, "attention_context": 512}
    z = {k: np.zeros((2, d), dtype=np.float32) for k, d in dims.items()}
    o = pkg.default_opts(dropout_seed=SEED)
    for n in sorted(STEPS):

        def hook():
            out, gt, gst = model.decoder_steps("persistent", mem, pm, nv, z, np.zeros((2, 80), dtype=np.float32), 0, n, o)
            return [out, gt] + [gst[k] for k in NAMES]

        got = with_stragglers(2, hook)
        for b in range(2):
            st = orc.new_state()
            oo = orc.default_opts(dropout_seed=SEED, item=b)
            ref = [orc.decoder_step(blob, c["enc"][b][0], c["enc"][b][1], nv[b], st, oo, s) for s in range(n)]
            assert rms(got[0][b], np.stack([r[0] for r in ref])) <= 1e-5
            assert np.abs(got[1][b] - np.array([r[1] for r in ref])).max() <= 1e-5
            for k, arr in zip(NAMES, got[2:]):
                want = np.array(getattr(st, NAMES[k]), dtype=np.float32)[: arr.shape[1]]
                assert np.abs(arr[b] - want).max() <= 1e-5, (k, T, b, n)
    assert model.engine_state()["decoder_persistent"] == 1
