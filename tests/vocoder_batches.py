"""Shared by test_vocoder_batches_cpu.py and test_gpu_vocoder_batches.py: how a ragged vocoder batch is packed into persistent
launches (csrc/gl_plan.h: gl_batch_pack, gl_batch_plan) restated in plain Python, the classes of plan a sweep has to reach, the
batches that reach them on a 256-CU device, and a model of what the request path does with a plan -- which rows every launch
reads and writes, which rows every fetch delivers -- against which the CPU test mutates the plan.

The rules restated here:

  an utterance rides     16 <= F, nb = ceil(F / tf) <= n_cu and F // nb >= 3; every other one runs alone, on its own call's engine
  packing                first-fit decreasing by nb (stable) over launches of n_cu * wg workgroups
  cost of a shape        launches x (4.85 | 6.0 | 6.1 for 4x1 | 4x2 | 8) + 6.1 per alone utterance of 16 frames or more
  shape                  4x2 where two fit a CU and it is cheaper than 4x1; 8 where batch_shape = 0 and it is cheaper than that;
                         then the developer switch: 8, 41, 42 (42 only where two fit)
  order                  the riders launch by launch, then the alone ones ascending: the row order of every record table
"""
from collections import namedtuple

import gl_shapes as gs

HOP = gs.HOP
COST_4X1, COST_4X2, COST_8 = 4.85, 6.0, 6.1   # gl_batch_pack: us per iteration of one launch of each shape
COST_ALONE = 6.1

Seg = namedtuple("Seg", "fbase F f0 n_own first last abase")
Plan = namedtuple("Plan", "TF WG riders room alone order segs seg0")


def rides(F, n_cu, tf):
    nb = -(-F // tf)
    return not (F < gs.TINY_BELOW or nb > n_cu or F // nb < gs.MIN_OWN)


def pack(Fu, n_cu, tf, wg):
    """gl_batch_pack: (cost, riders per launch, free workgroups per launch)."""
    items, n_alone = [], 0
    for u, F in enumerate(Fu):
        if not rides(F, n_cu, tf):
            n_alone += F >= gs.TINY_BELOW
            continue
        items.append((-(-F // tf), u))
    items.sort(key=lambda it: -it[0])  # (stable, as std::stable_sort)
    room, riders = [], []
    for nb, u in items:
        k = 0
        while k < len(room) and room[k] < nb:
            k += 1
        if k == len(room):
            room.append(n_cu * wg)
            riders.append([])
        room[k] -= nb
        riders[k].append(u)
    per = (COST_4X2 if wg > 1 else COST_4X1) if tf <= 4 else COST_8
    return per * len(riders) + COST_ALONE * n_alone, riders, room


def plan(Fu, n_cu, per_cu4, batch_shape, force):
    """gl_batch_plan: TF, WG, the riders and the free workgroups of each launch, the alone utterances, the row order, and the
    segment table with each launch's first row of it."""
    Fu = list(Fu)
    TF, WG = 4, 1
    riders, room, segs, seg0 = [], [], [], []
    if n_cu > 0:
        if per_cu4 >= 2 and pack(Fu, n_cu, 4, 2)[0] < pack(Fu, n_cu, 4, 1)[0]:
            WG = 2
        if batch_shape == 0 and pack(Fu, n_cu, gs.GLP_TF_MAX, 1)[0] < pack(Fu, n_cu, 4, WG)[0]:
            TF, WG = gs.GLP_TF_MAX, 1
        if force == 8:
            TF, WG = gs.GLP_TF_MAX, 1
        if force == 41:
            TF, WG = 4, 1
        if force == 42 and per_cu4 >= 2:
            TF, WG = 4, 2
        fbase, abase, f, a = [], [], 0, 0
        for F in Fu:
            fbase.append(f)
            abase.append(a)
            f += F
            a += HOP * (F - 1)
        _cost, riders, room = pack(Fu, n_cu, TF, WG)
        for utts in riders:
            seg0.append(len(segs))
            for u in utts:
                nb = -(-Fu[u] // TF)
                for b in range(nb):
                    f0, f1 = (b * Fu[u]) // nb, ((b + 1) * Fu[u]) // nb
                    segs.append(Seg(fbase[u], Fu[u], f0, f1 - f0, int(b == 0), int(b + 1 == nb), abase[u]))
    batched = {u for utts in riders for u in utts}
    alone = [u for u in range(len(Fu)) if u not in batched]
    order = [u for utts in riders for u in utts] + alone
    return Plan(TF, WG, [list(r) for r in riders], list(room), alone, order, segs, seg0)


def launch_of(p, n_utt):
    """what xdtts_griffinlim_batch_plan reports per utterance"""
    out = [-1] * n_utt
    for k, utts in enumerate(p.riders):
        for u in utts:
            out[u] = k
    return out


ALL_CLASSES = frozenset((
    "shape:4x1", "shape:4x2", "shape:8", "launches:1", "launches:2", "launches:3+", "launch:full", "launch:single-rider",
    "order:permuted", "alone:tiny", "alone:persistent", "alone:launch-engine", "alone:none", "later-launch:multi-utterance",
    "equal-length-neighbours"))


def classes(p, Fu, n_cu=256):
    """The names of what a plan exercises (n_cu: the device's, 0 for a handle without the persistent engine: it decides which
    engine an alone utterance gets)."""
    out = set()
    if p.riders:
        out.add("shape:8" if p.TF > 4 else "shape:4x%d" % p.WG)
        out.add("launches:%s" % (len(p.riders) if len(p.riders) < 3 else "3+"))
    if any(r == 0 for r in p.room):
        out.add("launch:full")
    if any(len(utts) == 1 for utts in p.riders):
        out.add("launch:single-rider")
    if p.order != list(range(len(Fu))):
        out.add("order:permuted")
    for u in p.alone:
        if Fu[u] < gs.TINY_BELOW:
            out.add("alone:tiny")
        elif n_cu > 0 and gs.plan(Fu[u], n_cu)[0] in ("p4", "p8"):
            out.add("alone:persistent")
        else:
            out.add("alone:launch-engine")
    if not p.alone:
        out.add("alone:none")
    if any(len(utts) >= 2 for utts in p.riders[1:]):
        out.add("later-launch:multi-utterance")
    if any(len({Fu[u] for u in utts}) < len(utts) for utts in p.riders):
        out.add("equal-length-neighbours")
    return out


# ---- the cases (at 256 CUs; test_vocoder_batches_cpu.py re-derives every plan quoted here) ---------------------------------------
CASES = {
    "A": (1000, 1001, 999, 5, 17),
    "B": (1024, 19, 1020, 16, 40, 1100, 2),
    "C": tuple(16 + (7 * i) % 23 for i in range(70)),
    "D": (600, 601, 37, 1500, 2100, 12, 203),
}
CASES["C30"] = CASES["C"][:30]   # the slice the magnitude-chain test runs
# form -> (batch_shape, XDTTS_GL_BATCH_FORCE)
FORMS = {"shape4": (4, None), "natural": (0, None), "41": (0, 41), "42": (0, 42), "8": (0, 8)}
# riders per launch at n_cu = 256, per_cu4 = 2
QUOTED = {
    ("A", "41"): [2, 1, 1], ("A", "42"): [3, 1], ("A", "8"): [3, 1],
    ("B", "41"): [1, 1, 3], ("B", "natural"): [4, 2],
    ("C", "41"): [29, 41], ("C", "42"): [70], ("C", "8"): [65, 5],
}
# A case that reaches no class of its own is kept only with its reason here (test_vocoder_batches_cpu.py asserts both).
JUSTIFIED = {
    "A": "the smallest batch with three launches whose first one is exactly full (251 + 5 workgroups), and three long "
         "utterances one frame apart: a neighbour's fbase or abase moves the audio by one hop, never by a whole utterance",
    "B": "the only case whose natural choice is the 8-frame shape with a full SECOND launch, and where F = 1100 leaves the "
         "4-frame batch for the single call's persistent engine while the same request's launches use the exchange buffer",
    "C": "the many-rows case of every record table (70 rows, 41 of them in a second launch), and the only one with two "
         "utterances of equal length in a LATER launch -- its classes are also C30's, which is a slice of it",
    "C30": "the slice of C the magnitude-chain test runs: one launch of one workgroup per CU that is not full, the only plan "
           "with a single launch on a device that admits one 4-frame workgroup per CU",
}


def case_plan(name, form, n_cu=256, per_cu4=2):
    shape, force = FORMS[form]
    return plan(CASES[name], n_cu, per_cu4, shape, force or 0)


def mels(name):
    """One seeded mel per utterance, keyed by its position: no two of a case are equal, whatever their F."""
    return [gs.speech_mel(F, seed=u) for u, F in enumerate(CASES[name])]


# ---- what the request path does with a plan: a model for the mutation checks ---------------------------------------------------
def simulate(p, Fu, content=None):
    """gl_batch_from_device on labels instead of numbers.  Frame row fbase[u] + f holds (content[u], f).  Each launch k runs
    the workgroups segs[seg0[k] .. + its nblk): a workgroup writes the hops f0 .. f0 + n_own of the audio at abase from the rows
    fbase + f0 ..; its fetch then delivers the rows tab_pos[first rider] .. + riders of the record tables, which follow `order`,
    and copies out its riders; the alone utterances follow one by one.  Returns, per utterance in the caller's order, (the
    labels of its audio, the labels its stats row was computed from); None marks what was never written."""
    n = len(Fu)
    content = list(range(n)) if content is None else content
    fbase, abase, f, a = [], [], 0, 0
    for F in Fu:
        fbase.append(f)
        abase.append(a)
        f, a = f + F, a + (F - 1)   # (in hops)
    rows = [None] * f
    for u in range(n):
        for k in range(Fu[u]):
            rows[fbase[u] + k] = (content[u], k)
    audio = [None] * a
    tab_pos = {u: r for r, u in enumerate(p.order)}
    delivered, out = {}, [None] * n

    def fetch(utts):
        r0 = tab_pos[utts[0]]
        for r in range(r0, r0 + len(utts)):
            if r < len(p.order):
                v = p.order[r]
                delivered[r] = tuple(audio[abase[v]:abase[v] + Fu[v] - 1])
        for u in utts:
            out[u] = delivered.get(tab_pos[u])

    nblk = [sum(-(-Fu[u] // p.TF) for u in utts) for utts in p.riders]
    for k, utts in enumerate(p.riders):
        for sg in p.segs[p.seg0[k]:p.seg0[k] + nblk[k]]:
            for h in range(sg.f0, min(sg.f0 + sg.n_own, sg.F - 1)):
                if sg.abase // HOP + h < len(audio):   # (a mutated plan may point past the end: lost in the model)
                    audio[sg.abase // HOP + h] = rows[sg.fbase + h]
        fetch(utts)
    for u in p.alone:
        for h in range(Fu[u] - 1):
            audio[abase[u] + h] = rows[fbase[u] + h]
        fetch([u])
    return [(out[u], delivered.get(tab_pos[u])) for u in range(n)]


def expected(Fu, content=None):
    content = list(range(len(Fu))) if content is None else content
    want = [tuple((content[u], h) for h in range(F - 1)) for u, F in enumerate(Fu)]
    return [(w, w) for w in want]


def mutate_swap_order(p, i, j):
    order = list(p.order)
    order[i], order[j] = order[j], order[i]
    return p._replace(order=order)


def mutate_drop_seg0(p, k):
    seg0 = list(p.seg0)
    seg0[k] = 0
    return p._replace(seg0=seg0)


def mutate_neighbour_abase(p, Fu, u, v):
    """utterances u and v (riders of one launch) take each other's abase"""
    fb, f = {}, 0
    for w, F in enumerate(Fu):
        fb[f] = w
        f += F
    ab = {}
    for sg in p.segs:
        ab[fb[sg.fbase]] = sg.abase
    swap = {u: ab[v], v: ab[u]}
    segs = [sg._replace(abase=swap.get(fb[sg.fbase], sg.abase)) for sg in p.segs]
    return p._replace(segs=segs)
