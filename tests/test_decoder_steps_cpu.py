"""The cases that test_gpu_decoder_steps.py sweeps reach every class the decoder engines take over the STEP axis -- how many steps
each chunk of a lock-step batch runs and where it stops --, every case reaches a class no other case does, the restated plan
(tests/decoder_steps.py) rests on the library's constants and agrees with a step-by-step model of the host loops for every
max_lim in 1..64, and the rigged gate of every gate-on case stops both oracles where the case says, with room.  This checks the
LIST and the oracles -- not the kernels."""
import os
import re
import time

import numpy as np

import decoder_steps as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr int %s = (\d+)[;,]" % name, text).group(1))


def test_the_restated_plan_uses_the_constants_and_the_lines_of_the_sources():
    handle_h, kernels, weights, dec, handle, p8 = (_src(n) for n in ("tacotron2_handle.h", "kernels.h", "weights.h", "tacotron2_decode.cpp",
                                                                     "tacotron2_handle.cpp", "decoder_persistent8.hip"))
    assert _const(handle_h, "GRAPH_STEPS") == ds.GRAPH_STEPS == 20
    assert "const int check_every = %d * GRAPH_STEPS;" % ds.CHECK_GRAPHS in dec and ds.CHECK_GRAPHS == 3
    assert _const(kernels, "PERSIST_B_MAX") == ds.PERSIST_B_MAX == 2 and _const(kernels, "P8_B_MAX") == ds.P8_B_MAX == 16
    assert _const(kernels, "PERSIST_T_MAX") == ds.PERSIST_T_MAX == 128 and _const(kernels, "P8_STEPS_MAX") == ds.P8_STEPS_MAX
    assert _const(weights, "BATCH_MFMA_MIN") == ds.BATCH_MFMA_MIN == 5
    assert re.search(r"NBMAX = (\d+),", p8).group(1) == str(ds.P8_NBMAX)
    # which engine
    assert "if (B < 3 || B > P8_B_MAX || T > PERSIST_T_MAX || max_steps > P8_STEPS_MAX) return false;" in dec
    assert "if (d.xf || d.B > 2 * PERSIST_B_MAX || d.T > PERSIST_T_MAX) return false;" in dec
    assert dec.count('env::equals(env::DECODER, "launch")') == 2 and "return p8_wanted &&" in dec
    assert "bool batched_mode = B >= BATCH_MFMA_MIN;" in handle and "batched_mode = !small_batch_engine(B, T, max_lim);" in handle
    # decode_launches
    assert "while (launched + GRAPH_STEPS <= max_lim) {" in dec and "r += r & 1;" in dec
    assert "for (int i = 0; i < check_every && launched < max_lim; i += GRAPH_STEPS) {" in dec
    assert "if (host_ctl[0] >= need || launched >= max_lim) break;" in dec
    assert "d.nframes[b] = limits[b];" in _src("decoder.hip")
    # decode_pairs
    assert "const int first = std::min(lim[b0], lim[b0 + 1]), r = lim[b0] > lim[b0 + 1] ? 0 : 1;" in dec
    assert "launch_decoder_persistent(view(b0 + r, 1), w, persist_view(g, r), lim[b0 + r] - first, stream);" in dec
    assert "if (g.shrink && !d.use_gate && lim[b0] == lim[b0 + 1]) {" in dec
    assert "if (b0 > 0) HIP_CHECK(hipMemsetAsync(d.ctl, 0, sizeof(int), stream));" in dec
    assert "launch_decoder_persistent(view(b0 + r, 1), w, g1, lim[b0 + r], stream);" in dec
    pers = _src("decoder_persistent.hip")
    assert "chunk 1 found stopped at its ph1(s) ->" in pers and "if (GATE && PB == 1 && !(step0 < d.nframes[0])) return;" in pers
    # the MFMA engine's slots and slabs
    assert "constexpr int p8_slots(int B) { return B <= 4 ? 4 : (B <= NBMAX ? NBMAX : P8_B_MAX); }" in p8
    assert "((size_t)(nsteps + 1) * PRENET + (size_t)nsteps * (ATT_RNN + EMB + DEC_RNN))" in p8
    # the batched sort, and the passes
    assert "return gate_off ? lim0[a] > lim0[c] : lens[a] > lens[c];" in handle and "std::stable_sort(order.begin(), order.end()," in handle
    assert "const int n0 = 64 * blockIdx.y;" in _src("decoder.hip") and ds.PASS_CHUNKS == 64
    assert "frames_dev + (size_t)b * frame_stride" in handle and "postnet_groups(d.frames, (size_t)d.max_steps * N_MEL," in handle


def test_which_engine_takes_a_request():
    e = ds.engine_for
    assert [e(B, 100, 40) for B in (1, 2, 3, 16, 17, 65)] == ["pair", "pair", "persistent8", "persistent8", "batched", "batched"]
    assert [e(B, 100, 40, "p8off") for B in (2, 3, 4, 5, 16)] == ["pair", "pair", "pair", "batched", "batched"]
    assert [e(B, 100, 40, "launch") for B in (1, 4, 5, 16)] == ["launch", "launch", "batched", "batched"]
    assert e(3, 129, 40) == "launch" and e(5, 129, 40) == "batched" and e(5, 100, ds.P8_STEPS_MAX + 1) == "batched"
    assert [ds.mfma_plan(ds.Case("x", "default", (2,) * B))["slots"] for B in (3, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16]


def test_every_class_is_reached_and_every_case_reaches_one_of_its_own():
    required = set(ds.REQUIRED)
    assert len(required) == len(ds.REQUIRED)
    own = {c.name: ds.classes(c) for c in ds.CASES}
    got = set().union(*own.values())
    print("%d cases reach %d classes, %d of them required" % (len(ds.CASES), len(got), len(required)))
    assert required <= got, sorted(required - got)
    for c in ds.CASES:
        rest = set().union(*(v for k, v in own.items() if k != c.name))
        # without this case a required class is lost ...
        assert not required <= rest or (c.name in ds.JUSTIFIED and len(ds.JUSTIFIED[c.name]) > 20), (c, "reaches no required class of its own and has no reason")
        # ... and no other case has the same set of classes
        same = [k for k, v in own.items() if k != c.name and v == own[c.name]]
        assert not same or c.name in ds.JUSTIFIED, (c, same)
        # the engine the case is meant for, and the sizing: caps <= 64, summed steps <= ~600
        assert max(c.ends) <= 64 and sum(c.ends) <= 600, (c, sum(c.ends))
    # every gate-less case of the persistent engines whose post-net is enqueued from the caps has a gate-on twin with the same counts
    on = {(c.form, c.ends) for c in ds.CASES if c.gate}
    for B in (3, 4, 5, 8, 9, 16):
        assert ("default", ds.BY_NAME["p8-off-B%d" % B].ends) in on
    for c in ds.CASES:
        if c.gate and c.B == 2:
            assert any(o.ends == c.ends and not o.gate and o.B == 2 for o in ds.CASES), c
    # call order: per engine a request and a longer one, both swept cases on the same form
    engines = set()
    for name, first, longer in ds.ORDER:
        a, b = ds.BY_NAME[first], ds.BY_NAME[longer]
        assert a.form == b.form and not a.gate and not b.gate and max(b.ends) > max(a.ends) and sum(b.ends) > sum(a.ends) and b.B >= a.B
        ea = ds.engine_for(a.B, ds.WINDOW, a.max_lim, a.form)
        assert ea == ds.engine_for(b.B, ds.WINDOW, b.max_lim, b.form)
        engines.add((ea, ds.mfma_plan(b)["slots"] if ea == "persistent8" else min(b.B, 2)))
    assert engines == {("launch", 2), ("batched", 2), ("pair", 2), ("pair", 1), ("persistent8", 8), ("persistent8", 16)}


def test_the_committed_figures_hold_one_entry_per_case():
    import json

    with open(os.path.join(ROOT, "profiles", "decoder_steps.json")) as f:
        rec = json.load(f)
    want = {"decoder_steps/" + c.name for c in ds.CASES} | {"decoder_steps/%s/decoder()" % c.name for c in ds.CASES if c.B == 1}
    assert set(rec) == want, sorted(set(rec) ^ want)
    for k, v in rec.items():
        c = ds.BY_NAME[k.split("/")[1]]
        assert v["engine"] == ds.engine_for(c.B, ds.WINDOW, c.max_lim, c.form) and 0.0 < v["err"] <= v["bound"] == 4.0 * v["d32"] + 1e-6, (k, v)


def _probes(max_lim):
    """requests around one max_lim, for the plan against the model: ragged caps, and stops with the gate on"""
    m = max_lim
    for form, B in (("launch", 3), ("p8off", 6), ("default", 17), ("default", 2), ("default", 1), ("p8off", 3), ("p8off", 4), ("default", 5)):
        caps = [m, max(m - 1, 1), 1, max(m // 2, 1), m, 2 if m > 1 else 1] + [1 + (7 * b) % m for b in range(11)]
        yield ds.Case("off", form, caps[:B])
        yield ds.Case("off-reversed", form, caps[:B][::-1])
        yield ds.Case("on", form, caps[:B], gate=True, max_steps=min(m + 3, 64))
        yield ds.Case("on-reversed", form, caps[:B][::-1], gate=True, max_steps=min(m + 3, 64))
        yield ds.Case("on-at-cap", form, caps[:B], gate=True, max_steps=m, fires=[c < m for c in caps[:B]])
        yield ds.Case("on-fires-at-cap", form, caps[:B], gate=True, max_steps=m)


def test_the_plan_agrees_with_the_step_by_step_model():
    """Every max_lim in 1..64, on every engine, gate off and on (a chunk at the cap with and without the gate firing there):
    the closed forms of decoder_steps.py against a literal walk through the host loops over a model of nframes[] and ctl[0]."""
    n = 0
    for max_lim in range(1, 65):
        for c in _probes(max_lim):
            engine = ds.engine_for(c.B, ds.WINDOW, c.max_lim, c.form)
            if engine in ("launch", "batched"):
                assert ds.launches_plan(c) == ds.launches_brute(c), (max_lim, c, c.ends, ds.launches_plan(c), ds.launches_brute(c))
            if engine == "batched":
                assert ds.batched_plan(c) == ds.batched_brute(c), (max_lim, c, c.ends)
            if engine == "pair":
                assert ds.pair_plan(c) == ds.pair_brute(c), (max_lim, c, c.ends, ds.pair_plan(c), ds.pair_brute(c))
            if engine == "persistent8":
                assert ds.mfma_plan(c)["steps"] == ds.mfma_brute(c) == max(c.ends)
            n += 1
    assert n == 64 * 8 * 6
    for c in ds.CASES:  # ... and at the swept cases themselves
        engine = ds.engine_for(c.B, ds.WINDOW, c.max_lim, c.form)
        if engine in ("launch", "batched"):
            assert ds.launches_plan(c) == ds.launches_brute(c), c
        if engine == "batched":
            assert ds.batched_plan(c) == ds.batched_brute(c), c
        if engine == "pair":
            assert ds.pair_plan(c) == ds.pair_brute(c), c
        if engine == "persistent8":
            assert ds.mfma_brute(c) == max(c.ends)


def test_the_plan_at_the_edges():
    lp = lambda *a, **k: ds.launches_plan(ds.Case("x", "launch", *a, **k))
    assert lp((19, 1)) == {"graphs": 0, "remainder": 20, "launched": 20, "idle": 1, "fetches": 1}
    assert lp((20, 1)) == {"graphs": 1, "remainder": 0, "launched": 20, "idle": 0, "fetches": 1}
    assert lp((21, 1)) == {"graphs": 1, "remainder": 2, "launched": 22, "idle": 1, "fetches": 1}
    assert lp((41, 40, 1))["graphs"] == 2 and lp((1, 1))["idle"] == 1 and lp((2, 1))["idle"] == 0
    assert lp((48, 30, 2), gate=True, max_steps=48, fires=(False, True, True)) == {"graphs": 3, "remainder": 0, "launched": 60, "idle": 12, "fetches": 2}
    assert lp((60, 21, 1), gate=True, max_steps=61)["launched"] == 60 and lp((21, 61, 2), gate=True, max_steps=61) == {"graphs": 4, "remainder": 0, "launched": 80, "idle": 19, "fetches": 3}
    pp = lambda *a, **k: ds.pair_plan(ds.Case("x", "default", *a, **k))
    assert pp((21, 21)) == [("pair", (0, 1), 0, (21, 21))]
    assert pp((21, 22)) == [("pair", (0, 1), 0, (21, 21)), ("one", (1,), 21, (1,))]
    assert pp((41, 21)) == [("pair", (0, 1), 0, (21, 21)), ("one", (0,), 21, (20,))]
    # gate on: chunk 1 first by one -- chunk 0 has completed its last step inside the pair launch, both continuations return at once
    assert pp((22, 21), gate=True) == [("pair", (0, 1), 0, (22, 21)), ("one", (0,), 22, (0,)), ("one", (1,), 22, (0,))]
    assert pp((22, 2), gate=True) == [("pair", (0, 1), 0, (3, 2)), ("one", (0,), 3, (19,)), ("one", (1,), 22, (0,))]
    assert pp((21, 22), gate=True) == [("pair", (0, 1), 0, (21, 21)), ("one", (0,), 21, (0,)), ("one", (1,), 21, (1,))]
    assert pp((1, 1), gate=True) == [("pair", (0, 1), 0, (1, 1)), ("one", (0,), 1, (0,)), ("one", (1,), 1, (0,))]
    four = ds.pair_plan(ds.Case("x", "p8off", (1, 2, 20, 41)))
    assert four == [("pair", (0, 1), 0, (1, 1)), ("one", (1,), 1, (1,)), ("pair", (2, 3), 0, (20, 20)), ("one", (3,), 20, (21,))]
    b = ds.batched_plan(ds.BY_NAME["batched-on-B17-last-tile-outlives"])
    assert b["tile_end"] == [6, 24] and not b["prefix"] and b["order"][-1] == 13
    assert ds.batched_plan(ds.BY_NAME["batched-on-B17-first-tile-outlives"])["tile_end"] == [24, 1]
    assert ds.batched_plan(ds.BY_NAME["batched-off-B65"])["passes"] == 2 and ds.batched_plan(ds.BY_NAME["batched-off-B17-odd"])["prefix"]
    assert ds.mfma_plan(ds.BY_NAME["p8-off-B16"]) == {"slots": 16, "kernel": "persistent16", "slabs": 22, "x_slabs": 23, "steps": 22}


def test_the_rigged_gate_stops_both_oracles_where_every_gate_on_case_says(orc, orc64, blob):
    """The condition of a gate-on case, on the oracles alone: with the gate_layer solved from the fp64 oracle's trajectory, the
    fp32 and the fp64 oracle stop every chunk at the designed frame (a chunk meant to run into max_steps: never) and no gate
    logit of either comes closer than GATE_ROOM = 0.005 to the threshold."""
    t0 = time.time()
    on = [c for c in ds.CASES if c.gate]
    assert len(on) >= 20
    worst = (np.inf,)
    for c in on:
        rig, room, slack, wmax = ds.rigged(orc, orc64, blob, c)  # (asserts the stops and the room)
        changed = np.nonzero(rig != blob)[0]
        assert 0 < len(changed) <= 1537 and changed.max() - changed.min() <= 1536  # gate_layer only: no frame changes
        print("rigged gate %-36s %2d chunks, %3d rows: room %.4f logits, solver slack %.4f, max |w| %.1f" % (c.name, c.B, sum(c.ends), room, slack, wmax))
        worst = min(worst, (room, c.name))
        assert room >= ds.GATE_ROOM and slack >= ds.GATE_ROOM
    print("closest gate of %d gate-on cases: %.4f logits (%s); %.1f s" % (len(on), worst[0], worst[1], time.time() - t0))
