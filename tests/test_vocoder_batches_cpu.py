"""The batches that test_gpu_vocoder_batches.py runs reach every way gl_batch_plan can pack a ragged vocoder batch into
persistent launches on a 256-CU device.  This checks the LIST and the restatement (tests/vocoder_batches.py against the constants
and expressions of csrc/gl_plan.h, and the plans the cases were chosen for), and that the comparison the GPU test makes would
see a wrong row order, a lost seg0 or a neighbour's abase -- which a batch of equal utterances does not."""
import os
import re

import gl_shapes as gs
import vocoder_batches as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")
N_CU = 256  # MI355X


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restatement_uses_the_constants_and_expressions_of_the_sources():
    plan = _src("gl_plan.h")
    pack = plan[plan.index("inline double gl_batch_pack("):plan.index("inline GlBatchPlan gl_batch_plan(")]
    assert "const int nb = (Fu[u] + tf - 1) / tf;" in pack
    assert "Fu[u] < %d || nb > n_cu || Fu[u] / nb < %d" % (gs.TINY_BELOW, gs.MIN_OWN) in pack
    assert "n_alone += Fu[u] >= %d;" % gs.TINY_BELOW in pack
    assert "std::stable_sort(" in pack and "return a.first > b.first;" in pack
    assert "while (k < room.size() && room[k] < it.first) ++k;" in pack and "room.push_back(n_cu * wg);" in pack
    m = re.search(r"return \(tf <= 4 \? \(wg > 1 \? ([\d.]+) : ([\d.]+)\) : ([\d.]+)\) \* \(double\)rd\.size\(\) \+ ([\d.]+) \* n_alone;", pack)
    assert m and [float(x) for x in m.groups()] == [vb.COST_4X2, vb.COST_4X1, vb.COST_8, vb.COST_ALONE]
    body = plan[plan.index("inline GlBatchPlan gl_batch_plan("):]
    assert "if (per_cu4 >= 2 && gl_batch_pack(Fu, n_cu, 4, 2) < gl_batch_pack(Fu, n_cu, 4, 1)) P.WG = 2;" in body
    assert "if (batch_shape == 0 && gl_batch_pack(Fu, n_cu, GLP_TF_MAX, 1) < gl_batch_pack(Fu, n_cu, 4, P.WG)) P.TF = GLP_TF_MAX, P.WG = 1;" in body
    assert "if (force == 8) P.TF = GLP_TF_MAX, P.WG = 1;" in body and "if (force == 41) P.TF = 4, P.WG = 1;" in body
    assert "if (force == 42 && per_cu4 >= 2) P.TF = 4, P.WG = 2;" in body
    assert "f += Fu[u], a += hop * (Fu[u] - 1), ++u) fbase[(size_t)u] = f, abase[(size_t)u] = a;" in body
    assert "sg.f0 = gl_fstart(b, Fu[u], nb);" in body and "sg.n_own = gl_fstart(b + 1, Fu[u], nb) - sg.f0;" in body
    assert "if (!P.batched[(size_t)u]) P.order.push_back(u);" in body
    assert int(re.search(r"constexpr int GLP_TF_MAX = (\d+);", plan).group(1)) == gs.GLP_TF_MAX
    # the request path and the plan query read the same arguments, through one helper
    handle, api = _src("griffinlim_handle.cpp"), _src("api_griffinlim.cpp")
    assert handle.count("gl_batch_args(g)") == 1 and api.count("gl_batch_args(g)") == 1
    assert handle.count("env::GL_BATCH_FORCE") == 1 and "env::GL_BATCH_FORCE" not in api
    for src in (handle, api):
        assert len(re.findall(r"gl_batch_plan\([^;]*a\.n_cu, \w+\.per_cu4, \w+\.batch_shape, \w+\.force\);", src)) == 1


def test_the_quoted_plans_hold():
    for (name, form), riders in vb.QUOTED.items():
        p = vb.case_plan(name, form, N_CU, 2)
        assert [len(r) for r in p.riders] == riders, (name, form, [len(r) for r in p.riders])
    A, B, C, D = (vb.CASES[k] for k in "ABCD")
    p = vb.case_plan("A", "41")
    assert p.riders == [[1, 4], [0], [2]] and p.room[0] == 0 and -(-1001 // 4) + -(-17 // 4) == 251 + 5 == N_CU
    assert p.alone == [3] and A[3] < gs.TINY_BELOW and p.order == [1, 4, 0, 2, 3]
    assert vb.case_plan("A", "42", N_CU, 1).TF == 8  # (where two do not fit a CU the switch 42 is not taken: the natural choice)
    p = vb.case_plan("B", "41")
    assert p.room[0] == 0 and p.riders[0] == [0] and p.alone == [5, 6] and gs.plan(B[5], N_CU)[0] == "p8" and B[6] < gs.TINY_BELOW
    p = vb.case_plan("B", "natural")
    assert p.TF == 8 and p.WG == 1 and p.room == [108, 0] and p.alone == [6]
    p = vb.case_plan("C", "41")
    assert p.room[0] == 0 and not p.alone and len(set(C)) == 23 and len(C) == 70
    assert vb.case_plan("C", "42").WG == 2
    for form in ("shape4", "41", "42"):
        p = vb.case_plan("D", form)
        assert p.alone == [3, 4, 5] and gs.plan(D[3], N_CU)[0] == "p8" and gs.plan(D[4], N_CU)[0] == "launch" and D[5] < gs.TINY_BELOW
    p = vb.case_plan("D", "8")
    assert p.alone == [4, 5] and 3 in p.riders[0]
    # every rider keeps the split of its own call under the 4-frame forms (what makes batch == single bit for bit possible)
    for name, Fu in vb.CASES.items():
        p = vb.case_plan(name, "41")
        at = 0
        for utts in p.riders:
            for u in utts:
                own = gs.plan(Fu[u], N_CU)[2]
                assert [s.n_own for s in p.segs[at:at + len(own)]] == own and gs.plan(Fu[u], N_CU)[0] == "p4", (name, u)
                at += len(own)
        assert at == len(p.segs)


def _union(per_cu4):
    own = {}
    for name, Fu in vb.CASES.items():
        own[name] = set()
        for form in vb.FORMS:
            own[name] |= vb.classes(vb.case_plan(name, form, N_CU, per_cu4), Fu, N_CU)
    return own


def test_the_cases_reach_every_class():
    own = _union(2)
    got = set().union(*own.values())
    assert got == vb.ALL_CLASSES, (sorted(vb.ALL_CLASSES - got), sorted(got - vb.ALL_CLASSES))
    # one 4-frame workgroup per CU: everything but the shape that needs two
    got1 = set().union(*_union(1).values())
    assert got1 == vb.ALL_CLASSES - {"shape:4x2"}, sorted(vb.ALL_CLASSES ^ got1)
    # every case is there for a class of its own, or has its reason
    for name in vb.CASES:
        rest = set().union(*(v for k, v in own.items() if k != name))
        assert rest != got or (name in vb.JUSTIFIED and len(vb.JUSTIFIED[name]) > 20), (name, "reaches no class of its own and has no reason")
    assert set(vb.JUSTIFIED) <= set(vb.CASES)
    # no handle without the persistent engine packs anything: every utterance alone, in the caller's order
    for name, Fu in vb.CASES.items():
        p = vb.plan(Fu, 0, 1, 0, 41)
        assert not p.riders and not p.segs and p.alone == p.order == list(range(len(Fu)))
        assert vb.classes(p, Fu, 0) <= {"alone:tiny", "alone:launch-engine"}


def test_no_two_utterances_of_a_case_are_equal():
    for name in vb.CASES:
        ms = vb.mels(name)
        assert [m.shape for m in ms] == [(80, F) for F in vb.CASES[name]]
        keys = {m.tobytes() for m in ms}
        assert len(keys) == len(ms), name
        # ... nor does one start with another (equal F or not): a neighbour's rows are never the right ones
        for i, a in enumerate(ms):
            for b in ms[i + 1:]:
                n = min(a.shape[1], b.shape[1])
                assert not (a[:, :n] == b[:, :n]).all(), name


def test_the_model_reproduces_the_request_on_every_plan():
    for name, Fu in vb.CASES.items():
        for form in vb.FORMS:
            for per_cu4 in (1, 2):
                p = vb.case_plan(name, form, N_CU, per_cu4)
                assert vb.simulate(p, Fu) == vb.expected(Fu), (name, form, per_cu4)
        assert vb.simulate(vb.plan(Fu, 0, 1, 0, 0), Fu) == vb.expected(Fu)


def test_the_comparison_sees_a_mutated_plan():
    """Each mutation changes what the GPU test compares (an utterance's audio or the stats it receives) on the cases' own,
    all-different utterances -- and on a batch of EQUAL utterances of one length, as 40 copies of one mel are, it does not:
    the blind spot this sweep closes."""
    for name in ("A", "C"):
        Fu = vb.CASES[name]
        want = vb.expected(Fu)
        p = vb.case_plan(name, "41")
        assert len(p.riders) >= 2
        # rows of two different fetches swapped: some utterance's rows are delivered by the wrong fetch
        i, j = 0, len(p.riders[0])
        assert vb.simulate(vb.mutate_swap_order(p, i, j), Fu) != want, name
        assert vb.simulate(vb.mutate_swap_order(p, 0, len(Fu) - 1), Fu) != want, name
        # ... and inside one fetch too: its first row is taken from its first rider
        if len(p.riders[0]) >= 2:
            assert vb.simulate(vb.mutate_swap_order(p, 0, 1), Fu) != want, name
        for k in range(1, len(p.riders)):
            assert vb.simulate(vb.mutate_drop_seg0(p, k), Fu) != want, (name, k)
        for utts in p.riders:
            for u, v in zip(utts, utts[1:]):
                assert vb.simulate(vb.mutate_neighbour_abase(p, Fu, u, v), Fu) != want, (name, u, v)
    # ... in particular between two utterances of EQUAL length in a LATER launch (case C holds such pairs)
    Fu = vb.CASES["C"]
    p = vb.case_plan("C", "41")
    pairs = [(u, v) for utts in p.riders[1:] for u in utts for v in utts if u < v and Fu[u] == Fu[v]]
    assert pairs
    for u, v in pairs:
        assert vb.simulate(vb.mutate_neighbour_abase(p, Fu, u, v), Fu) != vb.expected(Fu)
    # the blind spot: equal utterances hide exactly that mutation
    same = [0] * len(Fu)
    u, v = pairs[0]
    assert vb.simulate(vb.mutate_neighbour_abase(p, Fu, u, v), Fu, same) == vb.expected(Fu, same)
    old = [24] * 40 + [40] * 5   # the shape of the one multi-launch test there was: 40 copies of one mel and 5 of another
    content = [0] * 40 + [3] * 5
    for tf, wg in ((4, 1), (8, 1)):
        q = vb.plan(old, 24, 1, 0, 41 if tf == 4 else 8)   # (few CUs: several launches, as that test forces)
        assert len(q.riders) >= 2 and q.TF == tf
        a, b = [(u, v) for utts in q.riders[1:] for u, v in zip(utts, utts[1:]) if old[u] == old[v]][0]
        assert old[a] == old[b] and content[a] == content[b]
        assert vb.simulate(vb.mutate_neighbour_abase(q, old, a, b), old, content) == vb.expected(old, content)
        assert vb.simulate(vb.mutate_neighbour_abase(q, old, a, b), old) != vb.expected(old)


def test_the_plan_query_is_exported_and_checks_its_arguments(pkg):
    """xdtts_griffinlim_batch_plan: declared, bound, and a NULL handle or no utterance is an argument error before any device
    is looked at (the plans themselves: test_gpu_vocoder_batches.py, a handle needs a device)."""
    import ctypes as C

    assert "xdtts_griffinlim_batch_plan" in pkg.SYMBOLS and callable(pkg.GriffinLim.batch_plan)
    nf = (C.c_size_t * 2)(40, 17)
    assert pkg.lib.xdtts_griffinlim_batch_plan(None, nf, 2, *([None] * 6)) == pkg.XDTTS_ERR_BAD_ARG
    v = [C.c_int32(7) for _ in range(5)]
    assert pkg.lib.xdtts_griffinlim_batch_plan(None, nf, 0, *[C.byref(x) for x in v[:3]], None, *[C.byref(x) for x in v[3:]]) == pkg.XDTTS_ERR_BAD_ARG
    assert [x.value for x in v] == [7] * 5
