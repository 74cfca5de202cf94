"""Shared by test_decoder_steps_cpu.py and test_gpu_decoder_steps.py: what every decoder engine does with the STEP axis -- the
vector of per-chunk step caps lim[0..B) of a lock-step batch, and where each chunk stops -- restated in plain Python, a second,
step-by-step statement of the same, the cases that reach every class of that restatement, a gate rigged from the fp64 oracle
that stops every chunk of a case where the case says, and the references (fp64 oracle, and the fp32 oracle's own running
distance from it), computed once.

The rules restated here (csrc/tacotron2_decode.cpp, csrc/tacotron2_handle.cpp: infer_batch_device, csrc/decoder_persistent*.hip):

  which engine     3..16 chunks, T <= PERSIST_T_MAX, not XDTTS_DECODER=launch, not XDTTS_P8=0: the persistent MFMA engine; else from
                   BATCH_MFMA_MIN chunks the batched kernels on the launch-per-stage loop; else <= 2 PERSIST_B_MAX chunks, T <=
                   PERSIST_T_MAX, not XDTTS_DECODER=launch: the pair engine; else the launch-per-stage engine.
  decode_launches  gate off: a graph of GRAPH_STEPS steps while launched + GRAPH_STEPS <= max_lim, then one plain launch of the
                   remainder rounded up to even (`r += r & 1`): an odd max_lim runs one step with no chunk active.  Gate on: rounds
                   of three graphs while launched < max_lim, the counts fetched after each; a chunk still running reports its cap,
                   so the loop ends with the first round that covers the last stop -- launched overshoots in whole graphs.
  decode_pairs     chunks two at a time, ctl[0] reset between the launches.  One chunk: one launch.  Gate-less pair, equal caps:
                   one launch; unequal: a pair launch of min steps, the survivor's 1-chunk launch of lim - min from ctl[0].  Gate-on
                   pair: the skewed loop ends when either chunk is found stopped -- chunk 0 at its phase 1 of step s: both have run
                   s steps; chunk 1 at its phase 1 of step s: chunk 0 completes step s and has run s + 1 -- and the continuation of
                   BOTH chunks is enqueued blind: a stopped chunk's returns at once.
  MFMA engine      4 / 8 / 16 chunk slots for B <= 4 / <= 8 / <= 16; write-once rings of one slab per step, max_lim + 1 for x.
  batched          a stable sort, longest first: by cap with the gate off, by id count with the gate on (nothing then keeps the
                   running chunks a prefix of the 16-chunk tiles); more than 64 chunks take two passes of the MFMA kernels.
"""
import importlib.util
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import synth_ids
from gemm_shapes import bound, per_row_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPH_STEPS = 20       # csrc/tacotron2_handle.h
CHECK_GRAPHS = 3       # csrc/tacotron2_decode.cpp: check_every = 3 * GRAPH_STEPS
PERSIST_B_MAX = 2      # csrc/kernels.h
P8_B_MAX = 16          # csrc/kernels.h
P8_NBMAX = 8           # csrc/decoder_persistent8.hip (NBMAX: the 8-slot kernel)
P8_STEPS_MAX = 16384   # csrc/kernels.h
PERSIST_T_MAX = 128    # csrc/kernels.h
BATCH_MFMA_MIN = 5     # csrc/weights.h
TILE = 16              # chunks per MFMA tile of the batched kernels
PASS_CHUNKS = 64       # chunks per pass of the batched MFMA kernels

WINDOW = 100
DROPOUT_SEED = 29
MAX_STEPS_OFF = 64     # max_steps of the gate-less cases: the row stride of `frames`
GATE_ROOM = 0.005      # logits either side of the threshold a gate-on case must keep on both oracles
POOL = 8
FORMS = {"default": {}, "launch": {"XDTTS_DECODER": "launch"}, "p8off": {"XDTTS_P8": "0"}}
LENS = tuple(2 + (37 * b + 30) % 99 for b in range(65))  # ids of the chunk at batch position b: 2..100


def cdiv(a, b):
    return -(-a // b)


class Case:
    """One request: `ends[b]` frames of chunk b (gate off: its cap, passed as fixed_steps; gate on: where it stops), `fires[b]`:
    the gate stops it (else max_steps does), `lens[b]` its id count, `form` the switches the handle is created and called under."""

    def __init__(self, name, form, ends, gate=False, max_steps=None, fires=None, lens=None):
        self.name, self.form, self.gate = name, form, gate
        self.ends = tuple(int(e) for e in ends)
        self.B = len(self.ends)
        self.fires = tuple(fires) if fires is not None else (gate,) * self.B
        self.max_steps = max_steps if max_steps is not None else (max(self.ends) + 3 if gate else MAX_STEPS_OFF)
        self.lens = tuple(lens) if lens is not None else LENS[:self.B]
        self.lim = (self.max_steps,) * self.B if gate else self.ends
        self.max_lim = max(self.lim)
        assert len(self.lens) == len(self.fires) == self.B and all(1 <= n <= WINDOW for n in self.lens), name
        for e, f in zip(self.ends, self.fires):
            assert 1 <= e <= self.max_steps <= MAX_STEPS_OFF and (f or not gate or e == self.max_steps), name
        assert gate or not any(self.fires), name

    def chunks(self):
        """(id count, seed) of every chunk: the seed is the batch position, which is the dropout item too."""
        return [(n, b) for b, n in enumerate(self.lens)]

    def __repr__(self):
        return self.name


# ---- the plan restated ---------------------------------------------------------------------------------------------------

def engine_for(B, T, max_lim, form="default"):
    launch, p8 = form == "launch", form != "p8off"
    if 3 <= B <= P8_B_MAX and T <= PERSIST_T_MAX and max_lim <= P8_STEPS_MAX and not launch and p8:
        return "persistent8"
    if B >= BATCH_MFMA_MIN:
        return "batched"
    if B <= 2 * PERSIST_B_MAX and T <= PERSIST_T_MAX and not launch:
        return "pair"
    return "launch"


def engine_state_of(case):
    """What engine_state() of a fresh handle says after the case (-1: never probed, 0: off, 1: on): the MFMA engine is probed
    by every request of 3..16 chunks that XDTTS_DECODER=launch does not keep from it, the pair engine by every request that
    reaches use_persistent with row-major state and no XDTTS_DECODER=launch."""
    e = engine_for(case.B, WINDOW, case.max_lim, case.form)
    if e == "persistent8":
        return {"decoder_persistent8": 1}
    asked = 3 <= case.B <= P8_B_MAX and case.form != "launch"
    return {"decoder_persistent": 1 if e == "pair" else -1, "decoder_persistent8": 0 if asked else -1}


def launches_plan(case):
    """decode_launches: graphs replayed, the plain remainder launch, steps launched, steps with no chunk active, count fetches."""
    end, max_lim = max(case.ends), case.max_lim
    if not case.gate:
        graphs = max_lim // GRAPH_STEPS
        r = max_lim - graphs * GRAPH_STEPS
        r += r & 1
        launched = graphs * GRAPH_STEPS + r
        return {"graphs": graphs, "remainder": r, "launched": launched, "idle": launched - end, "fetches": 1}
    rounds = cdiv(end, CHECK_GRAPHS * GRAPH_STEPS)
    graphs = min(CHECK_GRAPHS * rounds, cdiv(max_lim, GRAPH_STEPS))
    return {"graphs": graphs, "remainder": 0, "launched": graphs * GRAPH_STEPS, "idle": graphs * GRAPH_STEPS - end, "fetches": rounds + 1}


def pair_plan(case):
    """decode_pairs: the launches as (kind, chunks, first step, steps each of its chunks runs)."""
    out = []
    for b0 in range(0, case.B, PERSIST_B_MAX):
        e = case.ends[b0:b0 + PERSIST_B_MAX]
        if len(e) == 1:
            out.append(("one", (b0,), 0, (e[0],)))
        elif not case.gate:
            first = min(e)
            out.append(("pair", (b0, b0 + 1), 0, (first, first)))
            if e[0] != e[1]:
                r = 0 if e[0] > e[1] else 1
                out.append(("one", (b0 + r,), first, (e[r] - first,)))
        else:
            ran0 = e[0] if e[0] <= e[1] else e[1] + 1  # chunk 1 found stopped: chunk 0 completes that step
            ctl = ran0
            out.append(("pair", (b0, b0 + 1), 0, (ran0, min(e))))
            for r in range(2):  # both continuations, blind
                n = max(0, e[r] - ctl)
                out.append(("one", (b0 + r,), ctl, (n,)))
                ctl += n
    return out


def mfma_plan(case):
    slots = 4 if case.B <= 4 else (P8_NBMAX if case.B <= P8_NBMAX else P8_B_MAX)
    return {"slots": slots, "kernel": "persistent16" if slots == P8_B_MAX else "persistent8<%d>" % slots, "slabs": case.max_lim,
            "x_slabs": case.max_lim + 1, "steps": max(case.ends)}


def batched_order(case):
    """order[j] = caller's index of the chunk in slot j (std::stable_sort, longest first)."""
    key = case.lens if case.gate else case.lim
    return sorted(range(case.B), key=lambda b: -key[b])


def batched_plan(case):
    order = batched_order(case)
    tile_end = [max(case.ends[b] for b in order[t:t + TILE]) for t in range(0, case.B, TILE)]
    return {"order": order, "tile_end": tile_end, "passes": cdiv(case.B, PASS_CHUNKS),
            "prefix": all(tile_end[t] >= tile_end[t + 1] for t in range(len(tile_end) - 1))}


# ---- the same, step by step: a model of the device (nframes, ctl[0]) under the host's loops -------------------------------

class _Device:
    def __init__(self, case):
        self.nf = list(case.lim)  # k_decoder_init: nframes[b] = limits[b]
        self.fire = [e - 1 if f else None for e, f in zip(case.ends, case.fires)]
        self.ctl = 0
        self.ran = [0] * case.B
        self.idle = 0

    def step(self, chunks):
        """one lock-step iteration of `chunks` at ctl[0]; False when none of them was active"""
        s, any_active = self.ctl, False
        for b in chunks:
            any_active |= self.step_of(b, s)
        self.ctl += 1
        self.idle += not any_active
        return any_active

    def step_of(self, b, s):
        if not s < self.nf[b]:
            return False
        self.ran[b] += 1
        if self.fire[b] == s:
            self.nf[b] = s + 1  # the tripping frame is kept
        return True


def launches_brute(case):
    dev, chunks, launched, graphs, r, fetches = _Device(case), range(case.B), 0, 0, 0, 0
    if not case.gate:
        while launched + GRAPH_STEPS <= case.max_lim:
            for _ in range(GRAPH_STEPS):
                dev.step(chunks)
            launched += GRAPH_STEPS
            graphs += 1
        if launched < case.max_lim:
            r = case.max_lim - launched
            r += r & 1
            for _ in range(r):
                dev.step(chunks)
            launched += r
        fetches = 1
    else:
        while True:
            i = 0
            while i < CHECK_GRAPHS * GRAPH_STEPS and launched < case.max_lim:
                for _ in range(GRAPH_STEPS):
                    dev.step(chunks)
                launched += GRAPH_STEPS
                graphs += 1
                i += GRAPH_STEPS
            fetches += 1
            if dev.ctl >= max(dev.nf) or launched >= case.max_lim:
                break
        fetches += 1
    assert tuple(dev.nf) == case.ends and tuple(dev.ran) == case.ends, (case, dev.nf, dev.ran)
    return {"graphs": graphs, "remainder": r, "launched": launched, "idle": dev.idle, "fetches": fetches}


def _kernel(dev, case, chunks, nsteps, shrink):
    """one launch of the persistent kernel from ctl[0] for at most nsteps; the steps each chunk ran"""
    s, ran = dev.ctl, [0] * len(chunks)
    stop = s + nsteps
    if len(chunks) == 1:
        b = chunks[0]
        if case.gate and not s < dev.nf[b]:
            return (0,)  # returns at once, ctl[0] as it was
        while s < stop and dev.step_of(b, s):
            s, ran[0] = s + 1, ran[0] + 1
    else:
        while s < stop:
            if shrink and not s < dev.nf[chunks[0]]:
                break  # chunk 0 found stopped at its phase 1 of step s: both have run s steps
            dev.step_of(chunks[0], s)
            ran[0] += 1
            if shrink and not s < dev.nf[chunks[1]]:
                s += 1  # chunk 1 found stopped: chunk 0 completes step s
                break
            dev.step_of(chunks[1], s)
            ran[1] += 1
            s += 1
    dev.ctl = s
    return tuple(ran)


def pair_brute(case):
    dev, out = _Device(case), []
    for b0 in range(0, case.B, PERSIST_B_MAX):
        n = min(PERSIST_B_MAX, case.B - b0)
        lim = case.lim[b0:b0 + n]
        dev.ctl = 0
        pair = tuple(range(b0, b0 + n))
        if n == 1:
            out.append(("one", pair, 0, _kernel(dev, case, pair, lim[0], False)))
        elif not case.gate:
            first = min(lim)
            out.append(("pair", pair, 0, _kernel(dev, case, pair, first, False)))
            if lim[0] != lim[1]:
                r = 0 if lim[0] > lim[1] else 1
                out.append(("one", (b0 + r,), dev.ctl, _kernel(dev, case, (b0 + r,), lim[r] - first, False)))
        else:
            out.append(("pair", pair, 0, _kernel(dev, case, pair, max(lim), True)))
            for r in range(n):
                start = dev.ctl
                out.append(("one", (b0 + r,), start, _kernel(dev, case, (b0 + r,), lim[r], False)))
    assert tuple(dev.nf) == case.ends and tuple(dev.ran) == case.ends, (case, dev.nf, dev.ran)
    return out


def mfma_brute(case):
    dev = _Device(case)
    while dev.ctl < case.max_lim and any(dev.ctl < n for n in dev.nf):  # ends early when every chunk has stopped
        dev.step(range(case.B))
    assert tuple(dev.nf) == case.ends and tuple(dev.ran) == case.ends and dev.idle == 0
    return dev.ctl


def batched_brute(case):
    """the tiles still live at every step, slot by slot"""
    key = case.lens if case.gate else case.lim
    order = list(range(case.B))
    for i in range(1, case.B):  # insertion sort: stable, longest first
        j = i
        while j > 0 and key[order[j - 1]] < key[order[j]]:
            order[j - 1], order[j] = order[j], order[j - 1]
            j -= 1
    n_tiles = cdiv(case.B, TILE)
    tile_end, prefix = [0] * n_tiles, True
    for s in range(max(case.ends)):
        live = [any(s < case.ends[b] for b in order[TILE * t:TILE * (t + 1)]) for t in range(n_tiles)]
        for t in range(n_tiles):
            if live[t]:
                tile_end[t] = s + 1
        prefix = prefix and all(live[t] or not live[t + 1] for t in range(n_tiles - 1))
    return {"order": order, "tile_end": tile_end, "passes": 1 + (case.B > PASS_CHUNKS), "prefix": prefix}


# ---- classes ---------------------------------------------------------------------------------------------------------------

SWEPT_MAX_LIM = (1, 2, 19, 20, 21, 39, 40, 41)


def classes(case):
    """The step-axis classes a case reaches, from the plans above; the sweep has to reach every string of REQUIRED."""
    engine = engine_for(case.B, WINDOW, case.max_lim, case.form)
    e, c, g = case.ends, set(), "on" if case.gate else "off"
    srt = sorted(e, reverse=True)
    if engine in ("launch", "batched"):
        p = launches_plan(case)
        if not case.gate:
            if engine == "launch" and case.max_lim in SWEPT_MAX_LIM:
                c.add("launch:off:max_lim=%d" % case.max_lim)
            if min(e) == 1 and case.B >= 2 and srt[1] == case.max_lim - 1:
                c.add("%s:off:ragged:min=1,second=max_lim-1" % engine)
            c.add("%s:off:graphs=%s" % (engine, p["graphs"] if p["graphs"] < 2 else "2+"))
            c.add("%s:off:remainder=%s" % (engine, "none" if p["remainder"] == 0 else ("rounded-up" if p["idle"] else "even")))
        else:
            if p["idle"] and max(e) == case.max_steps and case.max_steps % GRAPH_STEPS:
                c.add("%s:on:max_steps=%d:overshoot" % (engine, case.max_steps))
            if p["fetches"] == 2 and max(e) == CHECK_GRAPHS * GRAPH_STEPS and case.max_steps > max(e):
                c.add("%s:on:max_steps=%d:last-stop-at-%d:one-round" % (engine, case.max_steps, max(e)))
            if p["fetches"] == 3:
                c.add("%s:on:max_steps=%d:last-stop-at-%d:second-round" % (engine, case.max_steps, max(e)))
            if max(e) == 1:
                c.add("%s:on:all-stop-at-1" % engine)
            if sum(not f for f in case.fires) == 1 and case.B > 1:
                c.add("%s:on:one-at-cap" % engine)
    if engine == "batched":
        p = batched_plan(case)
        if case.gate and case.B == TILE + 1:
            if p["tile_end"][1] > p["tile_end"][0] and case.lens[p["order"][-1]] == min(case.lens):
                c.add("batched:on:B=17:last-tile-outlives-first")
            if p["tile_end"][1] == 1 and p["tile_end"][0] > 1:
                c.add("batched:on:B=17:first-tile-outlives-last")
        if not case.gate:
            if case.B == TILE + 1 and case.max_lim % 2:
                c.add("batched:off:B=17:odd-max_lim")
            if case.form == "p8off" and case.B <= P8_B_MAX:
                c.add("batched:off:p8off:B=%d" % case.B)
            if p["passes"] == 2:
                c.add("batched:off:two-pass")
    if engine == "pair":
        if case.B == 1:
            c.add("pair:B=1:%s:%d" % (g, e[0]))
        elif case.B == 2 and not case.gate:
            c.add("pair:off:min=%d:diff=%d:long=%d" % (min(e), abs(e[0] - e[1]), 0 if e[0] >= e[1] else 1))
        elif case.B == 2:
            plan = pair_plan(case)
            if not all(case.fires):
                c.add("pair:on:one-at-cap")
            elif max(e) == 1:
                c.add("pair:on:both-at-1")
            elif e[0] == e[1]:
                c.add("pair:on:same-frame")
            else:
                c.add("pair:on:chunk%d-first-by-%s" % (0 if e[0] < e[1] else 1, "1" if abs(e[0] - e[1]) == 1 else "many"))
            assert len(plan) == 3
        else:
            first, second = max(e[:2]), max(e[2:])
            c.add("pair:2x:B=%d:%s:longer-%s" % (case.B, g, "first" if first > second else "second"))
    if engine == "persistent8":
        p = mfma_plan(case)
        c.add("p8:slots=%d" % p["slots"])
        if max(e) == 1:
            c.add("p8:%s:all-1" % g)
        elif min(e) == 1:
            c.add("p8:%s:B=%d" % (g, case.B))
            if e[0] == max(e) and e.count(max(e)) == 1:
                c.add("p8:%s:longest-in-slot-0" % g)
            if e[-1] == max(e) and e.count(max(e)) == 1:
                c.add("p8:%s:longest-in-last-slot" % g)
    return frozenset(c)


REQUIRED = tuple(
    ["launch:off:max_lim=%d" % m for m in SWEPT_MAX_LIM]
    + ["launch:off:ragged:min=1,second=max_lim-1", "launch:off:remainder=rounded-up", "launch:off:remainder=even", "launch:off:remainder=none",
       "launch:off:graphs=0", "launch:off:graphs=1", "launch:off:graphs=2+",
       "launch:on:max_steps=48:overshoot", "launch:on:one-at-cap", "launch:on:max_steps=61:last-stop-at-60:one-round",
       "launch:on:max_steps=61:last-stop-at-61:second-round", "launch:on:all-stop-at-1"]
    + ["pair:B=1:%s:%d" % (g, n) for g in ("off", "on") for n in (1, 2, 21, 40)]
    + ["pair:off:min=%d:diff=%d:long=%d" % (m, d, r) for m in (1, 2, 21) for d in (0, 1, 2, 20) for r in ((0,) if d == 0 else (0, 1))]
    + ["pair:on:chunk0-first-by-1", "pair:on:chunk0-first-by-many", "pair:on:chunk1-first-by-1", "pair:on:chunk1-first-by-many",
       "pair:on:same-frame", "pair:on:both-at-1", "pair:on:one-at-cap"]
    + ["pair:2x:B=%d:off:longer-%s" % (B, w) for B in (3, 4) for w in ("first", "second")]
    + ["p8:%s:B=%d" % (g, B) for g in ("off", "on") for B in (3, 4, 5, 8, 9, 16)]
    + ["p8:%s:%s" % (g, k) for g in ("off", "on") for k in ("all-1", "longest-in-slot-0", "longest-in-last-slot")]
    + ["p8:slots=4", "p8:slots=8", "p8:slots=16"]
    + ["batched:on:B=17:last-tile-outlives-first", "batched:on:B=17:first-tile-outlives-last", "batched:off:B=17:odd-max_lim",
       "batched:off:p8off:B=6", "batched:off:p8off:B=12", "batched:off:two-pass", "batched:off:remainder=rounded-up"])


# ---- the cases -------------------------------------------------------------------------------------------------------------

def _ragged(B, max_lim, longest_at):
    """B caps: max_lim once, at `longest_at`; a 1 next to it; the rest 2 .. max_lim // 2 + 1"""
    caps = [2 + (5 * b) % (max_lim // 2) for b in range(B)]
    caps[longest_at] = max_lim
    caps[(longest_at + 1) % B] = 1
    return caps


def _cases():
    out = []
    # launch-per-stage engine, gate off: max_lim either side of one and two graphs, the smallest cap 1, the second max_lim - 1
    for m in SWEPT_MAX_LIM:
        out.append(Case("launch-off-%d" % m, "launch", (m, max(m - 1, 1), 1)))
    # ... gate on
    out.append(Case("launch-on-48-one-at-cap", "launch", (48, 30, 2), gate=True, max_steps=48, fires=(False, True, True)))
    out.append(Case("launch-on-61-stop-60", "launch", (60, 21, 1), gate=True, max_steps=61))
    out.append(Case("launch-on-61-stop-61", "launch", (21, 61, 2), gate=True, max_steps=61))
    out.append(Case("launch-on-all-1", "launch", (1, 1, 1), gate=True))
    # pair engine: one chunk
    for n in (1, 2, 21, 40):
        out.append(Case("one-off-%d" % n, "default", (n,)))
        out.append(Case("one-on-%d" % n, "default", (n,), gate=True))
    # gate-less pairs: the shorter chunk 1, 2, 21 steps, the longer 0, 1, 2, 20 more, either chunk the longer
    for m in (1, 2, 21):
        for d in (0, 1, 2, 20):
            for r in ((0,) if d == 0 else (0, 1)):
                out.append(Case("pair-off-%d+%d-long%d" % (m, d, r), "default", (m + d, m) if r == 0 else (m, m + d)))
    # gate-on pairs: each the twin of a gate-less one (same counts, the post-net enqueued from host_ctl instead of the caps)
    for e in ((21, 22), (2, 22), (22, 21), (22, 2), (21, 21), (1, 1)):
        out.append(Case("pair-on-%d-%d" % e, "default", e, gate=True))
    out.append(Case("pair-on-41cap-21", "default", (41, 21), gate=True, max_steps=41, fires=(False, True)))
    # 3 and 4 chunks as two pair launches
    out.append(Case("pairs-B3-longer-first", "p8off", (40, 21, 2)))
    out.append(Case("pairs-B3-longer-second", "p8off", (2, 1, 40)))
    out.append(Case("pairs-B4-longer-first", "p8off", (41, 20, 2, 1)))
    out.append(Case("pairs-B4-longer-second", "p8off", (1, 2, 20, 41)))
    # persistent MFMA engine: every slot count either side of its edges, the longest chunk first / last, gate off and its gate-on twin
    for B, m, at in ((3, 41, 0), (4, 40, 3), (5, 21, 0), (8, 22, 7), (9, 21, 0), (16, 22, 15)):
        for gate in (False, True):
            out.append(Case("p8-%s-B%d" % ("on" if gate else "off", B), "default", _ragged(B, m, at), gate=gate))
    out.append(Case("p8-off-all-1", "default", (1,) * 5))
    out.append(Case("p8-on-all-1", "default", (1,) * 5, gate=True))
    # batched engine.  Gate on, 17 chunks: the chunk of the fewest ids (caller's index 13, sorted last: alone in the second tile)
    lens17 = tuple(4 + 2 * ((5 * b + 3) % 17) for b in range(17))
    few, most = lens17.index(min(lens17)), lens17.index(max(lens17))
    ends = [2 + b % 5 for b in range(17)]
    ends[few] = 24
    out.append(Case("batched-on-B17-last-tile-outlives", "default", ends, gate=True, lens=lens17))
    ends = [3 + b % 5 for b in range(17)]
    ends[few], ends[most] = 1, 24
    out.append(Case("batched-on-B17-first-tile-outlives", "default", ends, gate=True, lens=lens17))
    out.append(Case("batched-off-B17-odd", "default", [1 + (4 * b) % 21 for b in range(17)]))
    out.append(Case("batched-off-p8off-B6", "p8off", (21, 20, 1, 7, 13, 2)))
    out.append(Case("batched-off-p8off-B12", "p8off", [40, 39, 1] + [2 + (3 * b) % 11 for b in range(9)]))
    out.append(Case("batched-off-B65", "default", [1 + (5 * b) % 12 for b in range(65)]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# call order on one handle, per engine: a request, a longer one, the first again
ORDER = (("launch", "launch-off-19", "launch-off-41"), ("batched", "batched-off-p8off-B6", "batched-off-p8off-B12"),
         ("pair", "pair-off-2+1-long1", "pair-off-21+20-long1"), ("one", "one-off-2", "one-off-40"),
         ("persistent8<8>", "p8-off-B5", "p8-off-B8"), ("persistent16", "p8-off-B9", "p8-off-B16"))
# a case whose classes another case reaches too, and why it stays
JUSTIFIED = {}


# ---- inputs, references and the rigged gate -----------------------------------------------------------------------------------

def ids_of(chunk):
    n, seed = chunk
    return synth_ids(n, seed=700 + seed)


_ENC, _REF, _RIG = {}, {}, {}


def _encoded(o, blob, chunk):
    key = (o.precision, chunk)
    if key not in _ENC:
        ids = np.zeros(WINDOW, dtype=np.int64)
        ids[:chunk[0]] = ids_of(chunk)
        _ENC[key] = o.encoder(blob, ids)
    return _ENC[key]


def reference(orc, orc64, blob, chunk, item, steps):
    """(fp64 mel (80, steps) of the chunk alone, d32: the fp32 oracle's distance from it per frame as the running maximum)."""
    key = (chunk, item, steps)
    if key not in _REF:
        m64 = orc64.infer_chunk(blob, ids_of(chunk), orc64.default_opts(fixed_steps=steps, dropout_seed=DROPOUT_SEED, item=item), window=WINDOW)
        m32 = orc.infer_chunk(blob, ids_of(chunk), orc.default_opts(fixed_steps=steps, dropout_seed=DROPOUT_SEED, item=item), window=WINDOW)
        assert m64.shape == m32.shape == (80, steps)
        d32 = np.maximum.accumulate(per_row_rel(m32, m64, 0))
        m64.setflags(write=False)
        d32.setflags(write=False)
        _REF[key] = (m64, d32)
    return _REF[key]


def references(orc, orc64, blob, case):
    """The references of a case's chunks on a few threads (the oracle runs outside the interpreter lock)."""
    with ThreadPoolExecutor(max_workers=POOL) as pool:
        return list(pool.map(lambda a: reference(orc, orc64, blob, a[1], a[0], case.ends[a[0]]), enumerate(case.chunks())))


def gate_rig():
    """xd-tts_amd/gate_rig.py from its file: the package itself would load the device library."""
    spec = importlib.util.spec_from_file_location("xdtts_gate_rig", os.path.join(ROOT, "xd-tts_amd", "gate_rig.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _trajectory(orc64, blob, chunk, item, n):
    """(n, 1536) rows [decoder_hidden ; attention_context] of the chunk's first n steps on the fp64 oracle."""
    mem, pm = _encoded(orc64, blob, chunk)
    st, opts = orc64.new_state(), orc64.default_opts(dropout_seed=DROPOUT_SEED, item=item)
    X = np.zeros((n, 1536), dtype=np.float64)
    for s in range(n):
        orc64.decoder_step(blob, mem, pm, chunk[0], st, opts, s)
        X[s, :1024] = np.ctypeslib.as_array(st.dec_h)
        X[s, 1024:] = np.ctypeslib.as_array(st.ctx)
    return X


def rigged(orc, orc64, blob, case):
    """(blob whose gate_layer stops chunk b of `case` after ends[b] frames -- never, if it does not fire --, the room in logits
    the closest gate of either oracle keeps from the threshold, the solver's slack and max |w|).  The condition of a gate-on
    case: both oracles stop every chunk at the designed frame with GATE_ROOM to spare; asserted here."""
    assert case.gate
    if case.name not in _RIG:
        gr = gate_rig()
        chunks = case.chunks()
        # a chunk that runs into max_steps gets one more row: its line crosses behind the last step the request runs
        n = [e if f else e + 1 for e, f in zip(case.ends, case.fires)]
        assert sum(n) < 1537, (case, sum(n))  # the fit is exact below 1537 equations
        with ThreadPoolExecutor(max_workers=POOL) as pool:
            X = list(pool.map(lambda b: _trajectory(orc64, blob, chunks[b], b, n[b]), range(case.B)))
        w, bias, slack, wmax = gr.solve_gate(X, n)
        rig = np.array(blob, dtype=np.float32)
        tab = {name: (off, numel) for name, _shape, off, numel in orc.tensor_table()}
        assert tab["gate_layer.weight"][1] == 1536 and tab["gate_layer.bias"][1] == 1
        rig[tab["gate_layer.weight"][0]:tab["gate_layer.weight"][0] + 1536] = w.astype(np.float32)
        rig[tab["gate_layer.bias"][0]] = np.float32(bias)
        rig.setflags(write=False)

        def room(args):
            o, b = args
            mem, pm = _encoded(o, blob, chunks[b])
            frames, gates = o.run_decoder(rig, mem, pm, chunks[b][0], o.default_opts(dropout_seed=DROPOUT_SEED, item=b, max_steps=case.max_steps))
            assert len(frames) == case.ends[b], (case, o.precision, b, len(frames), case.ends[b])
            below = gates[:-1] if case.fires[b] else gates
            r = float(gr.LOGIT_06 - below.max()) if len(below) else np.inf
            return min(r, float(gates[-1] - gr.LOGIT_06)) if case.fires[b] else r

        with ThreadPoolExecutor(max_workers=POOL) as pool:
            rooms = list(pool.map(room, [(o, b) for o in (orc, orc64) for b in range(case.B)]))
        assert min(rooms) >= GATE_ROOM, (case, min(rooms), slack)
        _RIG[case.name] = (rig, min(rooms), slack, wmax)
    return _RIG[case.name]


# ---- one GPU case --------------------------------------------------------------------------------------------------------------

class form_env:
    """the switches of a form, for the handle's creation (XDTTS_P8) and its requests (XDTTS_DECODER)"""

    def __init__(self, form):
        self.var = FORMS[form]

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.var}
        os.environ.update(self.var)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_case(pkg, handle, case):
    """the request of `case` on `handle` (created under the case's form, from the case's blob): the mels"""
    ids = [ids_of(c) for c in case.chunks()]
    with form_env(case.form):
        if case.gate:
            return handle.infer_batch(ids, opts=pkg.default_opts(dropout_seed=DROPOUT_SEED, max_steps=case.max_steps, max_chunk=WINDOW))
        return handle.infer_batch(ids, opts=pkg.default_opts(dropout_seed=DROPOUT_SEED, max_steps=case.max_steps, max_chunk=WINDOW),
                                  fixed_steps=np.asarray(case.ends, dtype=np.int32))


def compare(case, mels, refs):
    """every mel frame of every chunk against the fp64 oracle: (fails, the frame closest to its bound as (err / bound, err, d32
    (running maximum), bound, chunk, frame))"""
    fails, worst = [], None
    for b, (m64, d32) in enumerate(refs):
        if mels[b].shape != m64.shape or not np.all(np.isfinite(mels[b])):
            fails.append((b, "shape", mels[b].shape, m64.shape))
            continue
        e, bnd = per_row_rel(mels[b], m64, 0), bound(d32)
        t = int(np.argmax(e / bnd))
        w = (float(e[t] / bnd[t]), float(e[t]), float(d32[t]), float(bnd[t]), b, t)
        worst = w if worst is None or w > worst else worst
        for t in np.nonzero(e > bnd)[0][:4]:
            fails.append((b, int(t), float(e[t]), float(d32[t]), float(bnd[t])))
    return fails, worst
