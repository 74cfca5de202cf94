"""GPU parity of every decoder engine over the STEP axis: how many steps each chunk of a lock-step batch runs and where it stops
(tests/decoder_steps.py restates what the host loops of tacotron2_decode.cpp and infer_batch_device do with the caps and the
stop frames; test_decoder_steps_cpu.py shows that these cases reach every class of it, each case one of its own).  Everything
goes through the public entries -- infer_batch with fixed_steps per chunk, or with a gate rigged from the fp64 oracle's own
trajectory and max_steps; decoder() for one chunk -- because the graph replays, the survivor hand-off, the blind continuations,
the sort of a batch and the post-net enqueued from the caps are reachable in no other way.

Every mel frame of every chunk is compared with the fp64 oracle's infer_chunk of that chunk alone, per frame
|| gpu - f64 || / || f64 || (gemm_shapes.per_row_rel), against the project's bound

    err(gpu, f64) <= 4 d32 + 1e-6,   d32 = the fp32 oracle's distance from the fp64 oracle for the same chunk, as the running
                                     maximum over the frames up to the one compared

(gemm_shapes.bound; a lucky frame of the fp32 oracle does not tighten it).  Frame counts are exact.  Every case prints its figures
("decoder-steps ..." lines: pytest -rA shows them for passing tests too) and records them, under "decoder_steps/...", in the file
test_gpu_parity_regimes._report writes (those entries are committed as profiles/decoder_steps.json)."""
import numpy as np
import pytest

import decoder_steps as ds
from test_gpu_parity_regimes import _report

pytestmark = pytest.mark.gpu

LOGIT_06 = float(np.log(0.6 / 0.4))


def _handle(pkg, blob, form):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    with ds.form_env(form):
        return pkg.Tacotron2.from_blob(blob)


def _one_chunk_through_decoder(pkg, m, case):
    """B = 1 through the parity entry decoder(): the handle's own encoder output in, frames and delivered gate logits out"""
    ids = np.zeros(ds.WINDOW, dtype=np.int64)
    ids[:case.lens[0]] = ds.ids_of(case.chunks()[0])
    mem, pm = m.encoder(ids)
    kw = dict(max_steps=case.max_steps) if case.gate else dict(max_steps=case.max_steps, fixed_steps=case.ends[0])
    with ds.form_env(case.form):
        frames, gates = m.decoder(mem, pm, case.lens[0], pkg.default_opts(dropout_seed=ds.DROPOUT_SEED, **kw))
    assert frames.shape == (case.ends[0], 80) and gates.shape == (case.ends[0],), (case, frames.shape)
    assert m.last_timings()["steps"] == case.ends[0]
    if case.gate:  # the tripping frame is kept: its gate above the threshold, every earlier one below
        assert gates[-1] > LOGIT_06 and np.all(gates[:-1] <= LOGIT_06), (case, gates)
    return [m.postnet(frames)]


@pytest.mark.parametrize("name", [c.name for c in ds.CASES])
def test_every_chunk_runs_its_steps_and_matches_fp64(pkg, orc, orc64, blob, name):
    """One request per case on a fresh handle under the case's switches: frame counts equal to the fp64 oracle's chunk by chunk
    (gate on: the rigged gate stops both oracles there with 0.005 logits of room, asserted by decoder_steps.rigged), last_timings'
    steps the largest of them, every mel frame inside the bound, the engine the restated plan names.  A gate-less case of the
    persistent engines has the post-net enqueued from the caps before the counts come back; its gate-on twin (same counts, the
    post-net enqueued from host_ctl) is held to the same reference and bound.
    The sweep found no case outside the bound and no wrong count: the worst frame of a case stands at 0.07 .. 0.48 of its bound
    from 1 to 61 free-running steps.  Measured on an MI355X, the
    frame closest to its bound per engine, err(gpu, f64) | d32 | bound (the test prints every case):
      launch       3.53e-07 | 1.43e-07 | 1.57e-06 (launch-off-19, chunk 0, frame 9)
      batched      7.39e-07 | 1.33e-07 | 1.53e-06 (batched-off-B65, chunk 2, frame 5)
      pair         4.25e-07 | 1.48e-07 | 1.59e-06 (pairs-B3-longer-second, chunk 2, frame 25); decoder(): 3.75e-07 | 1.47e-07 | 1.59e-06 (one-off-40, frame 27)
      persistent8  4.31e-07 | 1.38e-07 | 1.55e-06 (p8-off-B16, chunk 14, frame 3)
    One-line errors tried on a scratch copy of the library, and the cases that caught each: the remainder launch not rounded up
    to even -- launch-off-1 / 19 / 21 / 39 / 41, batched-off-B17-odd, batched-off-p8off-B6; the survivor's launch one step short
    -- every gate-less pair with unequal caps and the four two-pair cases; only chunk 0's blind continuation -- pair-on-21-22,
    pair-on-2-22; the gate-on loop ended after its first fetch round -- launch-on-61-stop-61; the sorted batch without its
    dropout-stream permutation -- every batched case; the MFMA launch one step short -- every gate-less p8 case.  Two changed
    nothing a result can show: a pair launch of min + 1 steps (the kernel itself stops a chunk at its cap, the survivor starts
    at ctl[0]) and the gate-on batch sorted by cap (the order of the slots decides which tiles are skipped, not what they hold)."""
    case = ds.BY_NAME[name]
    refs = ds.references(orc, orc64, blob, case)
    weights = ds.rigged(orc, orc64, blob, case)[0] if case.gate else blob
    engine = ds.engine_for(case.B, ds.WINDOW, case.max_lim, case.form)
    m = _handle(pkg, weights, case.form)
    try:
        mels = ds.run_case(pkg, m, case)
        steps, st = m.last_timings()["steps"], m.engine_state()
        fails, worst = ds.compare(case, mels, refs)
        counts = [x.shape[1] for x in mels]
        print("decoder-steps %-36s %-11s B=%2d gate %-3s ends %s  worst frame err(gpu,f64) %.2e d32 %.2e bound %.2e err/bound %.3f (chunk %d, frame %d)  engines %s" % (
            case.name, engine, case.B, "on" if case.gate else "off", list(case.ends) if case.B <= 17 else "1..12 x 65",
            worst[1], worst[2], worst[3], worst[0], worst[4], worst[5], st) if worst else "decoder-steps %s: no chunk of the right shape" % case.name, flush=True)
        if worst:
            _report("decoder_steps/" + case.name, {"engine": engine, "err": worst[1], "d32": worst[2], "bound": worst[3], "chunk": worst[4], "frame": worst[5]})
        assert counts == list(case.ends), (case, counts, case.ends)
        assert steps == max(case.ends), (case, steps)
        assert not fails, (case, fails[:8])
        want = ds.engine_state_of(case)
        assert {k: st[k] for k in want} == want, (case, engine, st)
        if case.B == 1:
            f2, w2 = ds.compare(case, _one_chunk_through_decoder(pkg, m, case), refs)
            print("decoder-steps %-36s decoder()   worst frame err(gpu,f64) %.2e d32 %.2e bound %.2e (frame %d)" % (case.name, w2[1], w2[2], w2[3], w2[5]), flush=True)
            _report("decoder_steps/" + case.name + "/decoder()", {"engine": engine, "err": w2[1], "d32": w2[2], "bound": w2[3], "chunk": 0, "frame": w2[5]})
            assert not f2, (case, f2[:8])
    finally:
        m.close()


@pytest.mark.parametrize("engine,first,longer", ds.ORDER)
def test_a_request_after_a_longer_one_returns_the_bits_of_a_fresh_handle(pkg, blob, engine, first, longer):
    """Call order on one handle, per engine: a request, a longer one (more steps; on the batched and the MFMA engine more chunks
    too), the first again.  What a handle keeps across requests -- the captured graph, the exchange and its write-once rings with
    the longer request's slabs in them, the post-net's zero fills, the step caps on the device -- must not show: the repeated
    request returns the bits of its first run and of a fresh handle, and so does the longer one in between."""
    a, b = ds.BY_NAME[first], ds.BY_NAME[longer]
    m = _handle(pkg, blob, a.form)
    try:
        a1, b1, a2 = ds.run_case(pkg, m, a), ds.run_case(pkg, m, b), ds.run_case(pkg, m, a)
        want = ds.engine_state_of(b)
        assert {k: m.engine_state()[k] for k in want} == want, (engine, m.engine_state())
    finally:
        m.close()
    fresh = {}
    for c in (a, b):
        m = _handle(pkg, blob, c.form)
        try:
            fresh[c.name] = ds.run_case(pkg, m, c)
        finally:
            m.close()
    for what, got, ref, c in (("first run", a1, fresh[a.name], a), ("after the longer one", a2, a1, a), ("after the longer one, fresh handle", a2, fresh[a.name], a),
                              ("the longer one", b1, fresh[b.name], b)):
        assert [x.shape for x in got] == [(80, e) for e in c.ends], (engine, what)
        differ = [i for i, (x, y) in enumerate(zip(got, ref)) if not np.array_equal(x, y)]
        assert not differ, (engine, what, differ, [float(np.abs(got[i] - ref[i]).max()) for i in differ])
