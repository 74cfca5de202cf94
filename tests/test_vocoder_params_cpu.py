"""The grid of constructor parameters that test_gpu_vocoder_params.py sweeps reaches every K-slab class of k_gemm_nt and both
sides of the analysis projection's mapping flip; the kernel's operand fetch, restated in tests/vocoder_params.py, never
leaves its row (and the rule it replaced did, at K = 16); and every basis, power, momentum and iteration count of the grid
meets the oracle conditions the GPU rules rest on.  This checks the LISTS, the restatement against the text of the
sources, and the two CPU oracles -- not the kernels.  Figures are printed on "vocoder-params ..." lines (pytest -rA)."""
import os

import numpy as np
import pytest

import gemm_shapes as gs
import gl_shapes as gl
import vocoder_params as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_rules_are_the_text_of_the_sources():
    gemm = _src("gemm.hip")
    assert "const int lr = tid >> 3, lc = (tid & 7) * 4, lcs = lc < KL ? lc : 0;" in gemm
    assert "const int k0_ = ((SLAB) < nslab && (SLAB) * BK + lc < KL) ? (SLAB) * BK : 0;" in gemm
    assert gemm.count("k0_ =") == 1 and gemm.count("a_src[r_] + k0_") == 1 and gemm.count("b_src[r_] + k0_") == 1
    assert "const bool kok_ = (SLAB) * BK + lc < KL;" in gemm
    assert "a_src[r] = A + (size_t)(a_ok[r] ? m0 + lr + 32 * r : M - 1) * g.lda + kbeg + lcs;" in gemm
    assert "b_src[r] = g.W + (size_t)(b_ok[r] ? n0 + lr + 32 * r : g.N - 1) * g.K + kbeg + lcs;" in gemm
    assert gemm.count("a_src[") == 3 and gemm.count("b_src[") == 3  # declared, set once, read by GEMM_FETCH: nothing else moves them
    assert gemm.index("kbeg = ks * kper, KL = min(g.K - kbeg, kper);") < gemm.index("lcs = lc < KL ? lc : 0;")
    assert "const int kper = ((g.K + BK - 1) / BK + nks - 1) / nks * BK, kbeg = ks * kper, KL = min(g.K - kbeg, kper);" in gemm
    assert "const int nslab = (KL + BK - 1) / BK;" in gemm
    # the slabs GEMM_FETCH is asked for: the prologue's 0 .. 5, and s0 + J + 6 / + 4 from a step with s0 + J < nslab
    for s in range(6):
        assert "GEMM_FETCH(%d, q%d);" % (s, s % 4) in gemm
    assert gemm.count("GEMM_FETCH(s0 + (J) + 6, QA);") == 2 and gemm.count("GEMM_FETCH(s0 + (J) + 4, QB);") == 2
    assert gemm.count("GEMM_FETCH(") == 6 + 4 + 1  # (and the #define)
    assert "if (g.K % 16 != 0 || g.lda % 4 != 0) fail(" in gemm
    # the vocoder's call sites take their N / K / lda from the basis
    voc = _src("griffinlim_handle.cpp")
    for line in ("a.lda = n_mels;", "a.K = n_mels;", "r.N = n_mels;", "r.K = NBP;", "u.lda = n_mels;", "u.K = n_mels;", "a.N = g->n_mels;", "a.K = NBP;"):
        assert line in voc, line
    api = _src("api_griffinlim.cpp")
    assert 'if (n_mels % 16 != 0) fail(' in api and "!std::isfinite(power)" in api and "!std::isfinite(momentum)" in api
    syn = _src("api_synthesize.cpp")
    assert syn.count("pair_check(h, g);") == 3 and "if (g->n_mels != N_MEL) fail(XDTTS_ERR_BAD_ARG," in syn


def test_the_grid_reaches_every_slab_class_and_both_sides_of_the_flip():
    ks = sorted(vp.n_mels_of(k) for k in vp.BASES)
    classes = {vp.slab_class(K) for K in ks}
    print("vocoder-params grid K-slab classes %s" % sorted(classes))
    assert classes == {0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0}
    assert {vp.nslab(K) for K in ks} == {1, 2, 3, 4}          # the prologue's guarded 1 and 2, and the rounds' tail
    assert {(K // 16) % 2 for K in ks} == {0, 1}               # a half-full last slab, and a full one
    for K in ks:
        assert list(vp.slices_possible(K)) == [1]              # (no K of the grid could be split, and the vocoder never asks)
    # the sweeps' plans: every site on 32x32 tiles, the flips where the rules put them
    for key in vp.BASES:
        n = vp.n_mels_of(key)
        for F in vp.MEL2LIN_F:
            p = vp.plan(key, "mel2lin", F)
            assert p["tile"] == 32 and p["mapping"] == "plain" and p["slabs"] == (vp.nslab(n),), (key, F, p)
    for key, F in vp.MEL2LIN_XCD:
        assert vp.plan(key, "mel2lin", F)["mapping"] == "xcd" and vp.plan(key, "mel2lin", 513)["mapping"] == "plain"
    assert {k for k, _F in vp.MEL2LIN_XCD} == {"m16", "m128"}
    for key in vp.NNLS_BASES:
        lo, hi = vp.nnls_frames(key)
        assert lo >= 2 and [vp.plan(key, "nnls_res", F)["mapping"] for F in (lo, hi)] == ["plain", "xcd"], key
        assert all(vp.plan(key, "nnls_upd", F)["mapping"] == "plain" and vp.plan(key, "nnls_upd", F)["slabs"] == (vp.nslab(vp.n_mels_of(key)),) for F in (lo, hi))
    for key in vp.ANALYSIS_BASES:
        lo, hi = vp.analysis_frames(key)
        assert [vp.analysis_xcd(key, F) for F in (lo, hi)] == [False, True]
        assert [vp.plan(key, "analysis", F)["mapping"] for F in (lo, hi)] == ["plain", "xcd"], key
    assert {vp.n_mels_of(k) for k in vp.ANALYSIS_BASES} >= {16, 128} and {vp.n_mels_of(k) for k in vp.NNLS_BASES} >= {16, 128}
    # the loop's frame counts: the two-kernel path, and the persistent engine
    assert [gl.plan(F)[0] for F in vp.LOOP_F] == ["tiny", "p4", "p4"]
    assert set(vp.LOOP_MOMENTA) | {0.99} == set(vp.MOMENTA) and vp.ITERS == (0, 1, 2)
    # the control is the basis of every other test of the suite
    assert vp.BASES["m80"] == (gs.N_MEL, 8000.0) and vp.sites("m80") == {s: gs.SITES[s] for s in ("mel2lin", "nnls_res", "nnls_upd", "analysis")}


def test_the_fetch_never_leaves_its_row():
    """Every K the kernel accepts up to 2560 (the post-net's), every slice count the plan can return for it, every slab the
    pipeline asks for, every lane: the four columns lie in [0, K) of the lane's row, and what GEMM_STAGE keeps is each column of
    the slice once."""
    n = 0
    for K in range(16, 2561, 16):
        assert vp.fetch_violations(K) == [], K
        n += len(vp.slices_possible(K))
    assert {len(vp.slices_possible(K)) for K in (16, 496, 512, 768, 1024, 2560)} == {1, 2, 3, 4}
    print("vocoder-params fetch: %d (K, slices) pairs inside the row" % n)


def test_the_rule_before_the_fix_left_the_row_at_16_columns():
    """The same check pointed at the parent's rule (lc itself in the lane's base): at K = 16 the lanes with lc >= 16 load
    columns 16 .. 31 of a 16-column row -- the next row, and 64 bytes past the operand for the last one -- in all six slabs of the
    prologue; from K = 32 on that rule stays inside (lc + 3 <= 31 < K), so K = 16 is the one class it breaks."""
    bad = vp.fetch_violations(16, rule=vp.fetch_parent)
    assert bad and {c for *_x, c in bad} == {16, 20, 24, 28} and {t for _sk, _ks, _s, t, _c in bad} == {4, 5, 6, 7}
    assert {s for _sk, _ks, s, _t, _c in bad} == set(vp.fetched_slabs(16, 1, 0))
    assert max(c + 3 for *_x, c in bad) == 31  # 16 floats = 64 bytes past the row
    for K in range(32, 2561, 16):
        assert vp.fetch_violations(K, rule=vp.fetch_parent) == [], K
    # and the kept loads are the same under both rules: the fix changes no staged value
    for K in (16, 48, 80, 400, 528, 2560):
        for sk in vp.slices_possible(K):
            for ks in range(sk):
                for slab in vp.fetched_slabs(K, sk, ks):
                    for tid in range(8):
                        a, b = vp.fetch(K, sk, ks, slab, tid), vp.fetch_parent(K, sk, ks, slab, tid)
                        assert a[1] == b[1] and (not a[1] or a[0] == b[0])


@pytest.mark.parametrize("key", list(vp.BASES))
def test_every_basis_meets_the_oracle_conditions(orc, orc64, key):
    """Full rank with a moderate cond(B B^T), the fp32 and fp64 oracles' pseudo-inverses identical (both are fed the fp32 one
    anyway), and d32 of mel -> linear per frame at the powers of the grid small against the 1e-6 of the bound.  Measured:
    cond 14 .. 22 at fmax 8000 and 29 for the 11 025 Hz bank, d32 8e-8 .. 3e-7 at powers 1.0, 1.7 and 2.0 (0.6: up to 4.2e-7,
    the exponent 1 / 0.6 widens it)."""
    B, pinv = vp.basis_pinv(orc, key)
    n = vp.n_mels_of(key)
    assert B.shape == (n, vp.N_BINS) and pinv.shape == (vp.N_BINS, n) and n % 16 == 0
    g = B.astype(np.float64) @ B.astype(np.float64).T
    assert np.linalg.matrix_rank(g) == n
    cond = float(np.linalg.cond(g))
    assert np.array_equal(pinv, orc64.pinv(B))
    d = {}
    for power in vp.POWERS:
        d[power] = max(vp.mel2lin_ref(orc, orc64, key, F, power=power)[2] for F in vp.MEL2LIN_F)
    print("vocoder-params basis %-6s n_mels %3d K-slabs %.1f cond(B B^T) %5.1f  d32 of mel->linear at power %s" % (
        key, n, vp.slab_class(n), cond, "  ".join("%.1f: %.1e" % kv for kv in d.items())), flush=True)
    assert cond < 100.0, cond
    assert all(v < 2e-6 for v in d.values()), d


def test_the_rank_deficient_basis_is_one(orc):
    B = vp.rank_deficient_basis(orc)
    assert B.shape == (160, vp.N_BINS) and np.linalg.matrix_rank(B.astype(np.float64)) < 160
    with pytest.raises(ValueError):
        orc.pinv(B)


@pytest.mark.parametrize("key", vp.NNLS_BASES)
def test_nnls_and_power_mode_references(orc, orc64, key):
    """d32 of the refinement and of the other exponent conventions at the frame counts of the GPU sweep."""
    for F in vp.nnls_frames(key):
        for nnls, pm in vp.NNLS_MODES:
            d32 = vp.mel2lin_ref(orc, orc64, key, F, nnls_iters=nnls, power_mode=pm)[2]
            print("vocoder-params nnls-ref %-5s F=%3d nnls=%d power_mode=%d d32 %.2e" % (key, F, nnls, pm, d32), flush=True)
            assert d32 < 1e-5, (key, F, nnls, pm, d32)


def test_the_loop_references_keep_the_original_margin(orc, orc64):
    """check_audio's worst-hop bound of 1e-3 was set at 17 x what the fp32 oracle alone showed (5.7e-5): every loop, step and
    end-to-end case of the GPU module stays below 6e-5 there, so the margin is the original one.  And 0 iterations through
    the oracle's loop are the inverse STFT of S e^{i phase0}."""
    worst = 0.0
    for F in vp.LOOP_F:
        for mom in vp.MOMENTA:
            for it in vp.ITERS:
                S, p0, f32, f64 = vp.loop_ref(orc, orc64, F, mom, it)
                e, h = gl.rms(f32, f64), gl.worst_hop(f32, f64)
                print("vocoder-params loop-ref F=%2d momentum %.2f iters %d  f32-f64 rms %.2e  worst hop %.2e" % (F, mom, it, e, h), flush=True)
                assert h < vp.HOP_REF_MAX, (F, mom, it, h)
                worst = max(worst, h)
                if it == 0:
                    assert np.array_equal(f64, vp.istft_of_start(orc64, S, p0))
    for key in vp.BASES:
        Fs = (vp.E2E_F,) + (vp.BATCH_F if key in vp.BATCH_BASES else ())
        for F in Fs:
            _mel, f32, f64 = vp.e2e_ref(orc, orc64, key, F)
            e, h = gl.rms(f32, f64), gl.worst_hop(f32, f64)
            print("vocoder-params e2e-ref  %-6s F=%2d  f32-f64 rms %.2e  worst hop %.2e" % (key, F, e, h), flush=True)
            assert h < vp.HOP_REF_MAX, (key, F, h)
            worst = max(worst, h)
    print("vocoder-params loop-ref worst hop of all cases %.2e (limit %.0e)" % (worst, vp.HOP_REF_MAX))


def test_the_loop_cases_tell_the_parameters_apart(orc, orc64):
    """A handle that ignored its momentum or its iteration count would be caught: two iterations at momenta 0 / 0.5 / 0.99 lie
    5.7e-3 .. 1.5e-2 RMS apart, 0 / 1 / 2 iterations 3.6e-2 .. 1.2e-1 -- 50 x the 1e-4 the audio rule allows against the fp32
    oracle, and more.  (After one iteration from a zero previous spectrum the momentum has had nothing to act on: equal.)"""
    for F in vp.LOOP_F:
        r = {(m, i): vp.loop_ref(orc, orc64, F, m, i)[3] for m in vp.MOMENTA for i in vp.ITERS}
        for a, b in ((0.0, 0.5), (0.5, 0.99), (0.0, 0.99)):
            assert gl.rms(r[(a, 2)], r[(b, 2)]) > 5e-3, (F, a, b)
            assert np.array_equal(r[(a, 1)], r[(b, 1)]) and np.array_equal(r[(a, 0)], r[(b, 0)])
        for m in vp.MOMENTA:
            assert gl.rms(r[(m, 0)], r[(m, 1)]) > 5e-3 and gl.rms(r[(m, 1)], r[(m, 2)]) > 5e-3, (F, m)
    # and the bases: the end-to-end audio of one basis is not another's
    a = [vp.e2e_ref(orc, orc64, k, vp.E2E_F)[2] for k in vp.BASES]
    assert min(gl.rms(x, y) for i, x in enumerate(a) for y in a[:i]) > 5e-3


def test_the_step_references(orc, orc64):
    for F in vp.LOOP_F:
        for mom in vp.MOMENTA:
            _S, _a, _r, (oa, orr), (da, dr) = vp.step_ref(orc, orc64, F, mom)
            sig = float(np.sqrt(np.mean(dr ** 2)))
            print("vocoder-params step-ref F=%2d momentum %.2f  rebuilt rel f32-f64 %.2e  per frame %.2e  angles %.2e" % (
                F, mom, gl.rms(orr, dr) / sig, gl.per_frame_rel(orr, dr).max(), gl.rms(oa, da)), flush=True)
            assert gl.per_frame_rel(orr, dr).max() < 1e-5


@pytest.mark.parametrize("key", vp.ANALYSIS_BASES)
def test_the_analysis_references(orc, orc64, key):
    for F in vp.analysis_frames(key):
        _y, want, d32, m64, m32 = vp.analysis_ref(orc, orc64, key, F)
        assert want.shape == (vp.n_mels_of(key), F) and m64.shape == (vp.N_BINS, F)
        print("vocoder-params analysis-ref %-5s F=%3d d32 %.2e  smallest cell %.2e" % (key, F, d32, float(np.exp(want.min()))), flush=True)
        assert d32 < 1e-3
