"""The row counts that test_gpu_gemm_shapes.py sweeps reach every tile, block mapping, K split and slab loop that
k_gemm_nt can be given through the post-net, the encoder and mel -> linear.  This checks the LISTS (against
tests/gemm_shapes.py's restatement of the plan, and that restatement against the text of the sources), the fp64
numpy post-net against the oracle, and what the per-row metric and the bound can see -- not the kernels."""
import os
import re
import time

import numpy as np
import pytest

import gemm_shapes as gs
from conftest import synth_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xd-tts_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    return int(re.search(r"constexpr int %s = (\d+)[;,]" % name, text).group(1))


def test_the_restated_rules_use_the_constants_of_the_sources():
    gemm, common, kernels = _src("gemm.hip"), _src("common.h"), _src("kernels.h")
    assert _const(gemm, "BK") == gs.BK == 32
    # the 64x64 rule stands twice (the launcher and the split plan must agree on it): the same text both times
    big = "g.N >= 64 && tiles64 >= 512 && !(g.M <= 128 && g.N >= 4096)"
    tiles64 = "const long tiles64 = (long)((g.N + 63) / 64) * ((g.M + 63) / 64) * g.batch;"
    assert gemm.count(big) == 2 and gemm.count(tiles64) == 2
    assert "const bool big = %s;" % big in gemm                                  # gemm_splitk_plan
    assert "(forced ? forced == 64 : (%s))" % big in gemm and "g.tile ? g.tile == 64 :" in gemm  # launch_gemm_nt
    xcd = "rows * g.lda > (long)g.N * g.K"
    assert "if (big || %s) return 1;" % xcd in gemm and "a.xcd_rows = %s ? 1 : 0;" % xcd in gemm
    assert "t32 += (long)((m + 31) / 32) * ((g.N + 31) / 32);" in gemm and "const int tb = forced_t ? forced_t : 32;" in gemm
    assert "(int)std::min<long>(4, 512 / std::max<long>(blocks, 1))" in gemm
    assert "sk = std::min(sk, nslab / 8);" in gemm and "if (sk < 2) return 1;" in gemm
    assert "const int nslab = (g.K + 31) / 32;" in gemm
    assert "const int kper = ((g.K + BK - 1) / BK + nks - 1) / nks * BK, kbeg = ks * kper, KL = min(g.K - kbeg, kper);" in gemm
    assert "for (; s0 + 14 <= nslab; s0 += 12) {" in gemm and "ny = (int)((tiles + 7) / 8 * 8);" in gemm
    assert "if (a.splitk > 1 && (a.xcd_rows || !a.ws || !a.cnt)) a.splitk = 1;" in gemm
    assert "static constexpr int NBP = %d;" % gs.NBP in _src("griffinlim_handle.h") and gs.NBP == 528
    assert _const(common, "T_MAX") == gs.T_MAX == 512 and _const(kernels, "GEMM_RAGGED_MAX") == gs.GEMM_RAGGED_MAX == 64
    # only the Tacotron2 handle splits K: every GEMM of its handle file goes through run_gemm, the vocoder's never plan
    voc = _src("griffinlim_handle.cpp")
    assert "gemm_splitk_plan" not in voc
    for name in ("api_griffinlim.cpp", "api_gl_magnitude.cpp", "api_gl_delivery.cpp", "delivery.cpp"):
        assert "gemm_splitk_plan" not in _src(name), name
    assert voc.count("launch_gemm_nt(") == 5 and voc.count("a.tile = 32;") == 1 and voc.count(".tile = ") == 1
    taco = _src("tacotron2_handle.cpp")
    assert taco.count("gemm_splitk_plan(") == 1 and taco.count("launch_gemm_nt(") == 1 and taco.count("run_gemm(g);") == 4
    # the table of call sites: N, K, lda from the model's dimensions
    emb, enc_k, enc_h, att = _const(common, "EMB"), _const(common, "ENC_K"), _const(common, "ENC_H"), _const(common, "ATT_DIM")
    mel, ch, post_k = _const(common, "N_MEL"), _const(common, "POST_CH"), _const(common, "POST_K")
    want = {"post0": (ch, post_k * mel, mel), "post13": (ch, post_k * ch, ch), "post4": (mel, post_k * ch, ch),
            "enc_conv": (emb, enc_k * emb, emb), "bilstm_proj": (4 * enc_h, emb, emb), "memory": (att, emb, emb),
            "mel2lin": (gs.N_BINS, mel, mel), "nnls_res": (mel, gs.NBP, gs.NBP), "nnls_upd": (gs.NBP, mel, mel), "analysis": (mel, gs.NBP, gs.NBP)}
    assert {k: (v["N"], v["K"], v["lda"]) for k, v in gs.SITES.items()} == want
    assert [k for k, v in gs.SITES.items() if v["split"]] == ["post0", "post13", "post4", "enc_conv", "bilstm_proj", "memory"]
    assert [k for k, v in gs.SITES.items() if v["tile"]] == ["analysis"] and gs.SITES["analysis"]["tile"] == 32
    assert all(v["K"] % 16 == 0 and v["lda"] % 4 == 0 for v in gs.SITES.values())  # what launch_gemm_nt accepts


def _p(site, M, *keys):
    p = gs.plan(site, M)
    return tuple(p[k] for k in keys)


def test_plan_at_the_thresholds():
    K = ("tile", "mapping", "slices", "slabs")
    for site in ("post13", "enc_conv"):  # 80 slabs
        assert _p(site, 1, *K) == _p(site, 256, *K) == (32, "plain", 4, (20, 20, 20, 20))
        assert _p(site, 257, *K) == _p(site, 320, *K) == (32, "plain", 3, (27, 27, 26))
        assert _p(site, 321, *K) == _p(site, 512, *K) == (32, "plain", 2, (40, 40))
        assert _p(site, 513, *K) == _p(site, 2560, *K) == (32, "plain", 1, (80,))
        assert _p(site, 2561, *K) == _p(site, 4032, *K) == (32, "xcd", 1, (80,))
        assert _p(site, 4033, *K) == (64, "xcd", 1, (80,))
    for M in (1, 512, 2560):  # layer 0: 13 slabs, the last a half slab, never split
        assert _p("post0", M, *K) == (32, "plain", 1, (13,))
    assert _p("post0", 2561, *K) == _p("post0", 4032, *K) == (32, "xcd", 1, (13,)) and _p("post0", 4033, *K) == (64, "xcd", 1, (13,))
    assert gs.SITES["post0"]["K"] % gs.BK == 16
    assert _p("post4", 1, *K) == _p("post4", 400, *K) == (32, "plain", 4, (20, 20, 20, 20))
    assert _p("post4", 401, *K) == _p("post4", 4100, *K) == (32, "xcd", 1, (80,))
    assert gs.plan("post4", 400)["col_tiles"] == 3 and gs.SITES["post4"]["N"] % 32 == 16  # the last column tile half full
    assert _p("bilstm_proj", 1, *K) == _p("bilstm_proj", 256, *K) == (32, "plain", 2, (8, 8))
    assert _p("bilstm_proj", 257, *K) == _p("bilstm_proj", 512, *K) == (32, "plain", 1, (16,))
    assert _p("memory", 1, *K) == _p("memory", 128, *K) == (32, "plain", 2, (8, 8))
    assert _p("memory", 129, *K) == _p("memory", 512, *K) == (32, "xcd", 1, (16,))
    assert _p("mel2lin", 1, *K) == _p("mel2lin", 513, *K) == (32, "plain", 1, (3,))
    assert _p("mel2lin", 514, *K) == _p("mel2lin", 3584, *K) == (32, "xcd", 1, (3,)) and _p("mel2lin", 3585, *K) == (64, "xcd", 1, (3,))
    assert gs.plan("mel2lin", 1)["col_tiles"] == 17 and gs.SITES["mel2lin"]["N"] % 32 == 1  # the last column tile 1 wide
    assert _p("nnls_res", 80, *K) == (32, "plain", 1, (17,)) and _p("nnls_res", 81, *K) == _p("nnls_res", 3700, *K) == (32, "xcd", 1, (17,))
    assert _p("analysis", 80, *K) == (32, "plain", 1, (17,)) and _p("analysis", 81, *K) == _p("analysis", 100000, *K) == (32, "xcd", 1, (17,))
    assert _p("nnls_upd", 528, *K) == (32, "plain", 1, (3,)) and _p("nnls_upd", 529, *K) == _p("nnls_upd", 3584, *K) == (32, "xcd", 1, (3,))
    assert _p("nnls_upd", 3585, *K) == (64, "xcd", 1, (3,))
    # the XCD mapping's grid: row tiles rounded up to 8, the rest of the last group exits
    assert _p("post13", 2561, "row_tiles", "padded") == (81, True) and _p("post13", 4033, "row_tiles", "padded") == (64, False)
    assert _p("post4", 401, "row_tiles", "padded") == (13, True) and _p("post4", 512, "row_tiles", "padded") == (16, False)
    # the forced-tile child: 64x64 everywhere, no split; the analysis projection keeps its own 32
    assert gs.plan("post13", 130, force_tile=64, force_nosplit=True)["tile"] == 64 and gs.plan("post13", 130, force_nosplit=True)["slices"] == 1
    assert gs.plan("analysis", 130, force_tile=64)["tile"] == 32
    # every slice keeps the 8 slabs the pipeline's prologue needs, and the slices cover K exactly once
    for site, s in gs.SITES.items():
        for M in (1, 100, 256, 257, 400, 401, 512):
            p = gs.plan(site, M)
            assert sum(p["slabs"]) == gs.cdiv(s["K"], gs.BK) and (p["slices"] == 1 or min(p["slabs"]) >= 8), (site, M, p)
            assert p["slices"] == 1 or (p["mapping"] == "plain" and p["tile"] == 32), (site, M, p)


# Classes no sweep reaches, each with its reason.  Nothing else may be missing.
_XCD32 = ("32x32 under the XCD mapping at N = 512 between 2561 and 4032 rows: a fp64 reference of 4-6 s each; F = 2561 runs this mapping and "
          "grid width, and every last-tile kind and group fill runs under the same mapping on layer 4 (401, 416, 481, 500, 512, 520)")
_T64 = ("natural 64x64 past 4033 rows: 6 s of fp64 reference each; F = 4033 runs the natural 64x64 launch, the forced-tile child runs every "
        "last-tile kind of 64x64 (F = 16, 17, 33, 49, 64, 65, 130)")
LEFT_OUT = {}
for _site, _slabs in (("post0", "13"), ("post13", "80")):
    for _kind in ("gt16:groups-padded", "full:groups-padded", "le16:groups-of-8", "gt16:groups-of-8", "full:groups-of-8"):
        LEFT_OUT["%s:t32:xcd:s1:%s:%s" % (_site, _slabs, _kind)] = _XCD32
    for _kind in ("le32:groups-of-8", "le48:groups-of-8", "gt48:groups-of-8", "full:groups-of-8", "le16:groups-padded"):
        LEFT_OUT["%s:t64:xcd:s1:%s:%s" % (_site, _slabs, _kind)] = _T64


def test_the_sweeps_reach_every_class():
    every = {e: gs.entry_classes(e, rng) for e, (_, rng) in gs.ENTRIES.items()}
    got = {
        "postnet": gs.entry_classes("postnet", gs.SWEEP_POSTNET),
        "encoder": gs.entry_classes("encoder", gs.SWEEP_ENCODER),
        # nnls_iters = 0 runs the first product alone; with the refinement all three run
        "mel_to_linear": gs.entry_classes("mel_to_linear", gs.SWEEP_MEL2LIN + gs.SWEEP_NNLS, ("mel2lin",))
        | gs.entry_classes("mel_to_linear", gs.SWEEP_NNLS, ("nnls_res", "nnls_upd")),
    }
    missing = set()
    for e in every:
        assert got[e] <= every[e], (e, sorted(got[e] - every[e]))
        missing |= every[e] - got[e]
    assert missing == set(LEFT_OUT), (sorted(missing - set(LEFT_OUT)), sorted(set(LEFT_OUT) - missing))
    assert all(len(r) > 20 for r in LEFT_OUT.values()) and len(LEFT_OUT) == 20
    assert every["encoder"] == got["encoder"] and every["mel_to_linear"] == got["mel_to_linear"]  # nothing left out there
    assert not any(c.startswith("post4") for c in LEFT_OUT)
    # what the left-out classes lean on is really swept
    small = [gs.shape_class("post4", F).split(":", 1)[1] for F in (401, 416, 520, 481, 500, 512)]
    assert small == ["t32:xcd:s1:80:%s" % k for k in ("gt16:groups-padded", "full:groups-padded", "le16:groups-padded", "le16:groups-of-8", "gt16:groups-of-8", "full:groups-of-8")]
    assert {401, 416, 520, 481, 500, 512} <= set(gs.SWEEP_POSTNET)
    forced = {gs.last_row_tile(F, 64) for F in gs.FORCED64_POSTNET}
    assert forced == {"le16", "le32", "le48", "gt48", "full"} and {gs.last_row_tile(F, 64) for F in gs.FORCED64_MEL2LIN} == {"le16", "le32", "gt48"}
    # the analysis projection: plain at 80 rows, the XCD mapping after, groups padded and of 8
    assert [gs.shape_class("analysis", F).split(":", 2)[2] for F in gs.SWEEP_ANALYSIS] == [
        "plain:s1:17:le16", "xcd:s1:17:gt16:groups-padded", "xcd:s1:17:gt16:groups-padded", "xcd:s1:17:le16:groups-padded"]
    # the call-order lists
    assert set(gs.ORDER_POSTNET) == {F for F in gs.SWEEP_POSTNET if F <= gs.SMALL} | {37} and len(set(gs.ORDER_POSTNET)) == len(gs.ORDER_POSTNET)
    assert set(gs.FRESH_POSTNET) <= set(gs.ORDER_POSTNET) and set(gs.FRESH_ENCODER) <= set(gs.ORDER_ENCODER)
    assert {gs.plan("post13", F)["slices"] for F in gs.ORDER_POSTNET} == {1, 2, 3, 4} and {gs.plan("post4", F)["mapping"] for F in gs.ORDER_POSTNET} == {"plain", "xcd"}
    assert {gs.plan("enc_conv", T)["slices"] for T in gs.ORDER_ENCODER} == {2, 4}


def test_the_numpy_postnet_is_the_fp64_oracles(orc, orc64, blob):
    for F in (1, 3, 37, 100):
        fr = gs.postnet_frames(F)
        want, got = orc64.postnet(blob, fr), gs.postnet_numpy(orc, blob, fr)
        assert got.shape == want.shape == (80, F) and got.dtype == np.float64
        e = gs.worst(got, want, 0)
        ec = gs.worst(got - fr.T, want - fr.T, 0)
        print("numpy post-net F=%d: per frame %.2e, on the contribution %.2e" % (F, e, ec))
        assert e <= 1e-12 and ec <= 1e-12, (F, e, ec)
    # the stack's own contribution is a tenth of the output, so an RMS of the whole mel hides its errors ten times over
    fr = gs.postnet_frames(100)
    out = orc64.postnet(blob, fr)
    c, o = gs.rms(out - fr.T, 0 * out), gs.rms(out, 0 * out)
    print("contribution rms %.3f, output rms %.3f" % (c, o))
    assert 0.05 < c < 0.2 and 0.9 < o < 1.1


def test_per_row_rel_sees_one_column_taken_from_its_neighbour():
    rng = np.random.default_rng(0)
    F = 4033
    ref = rng.standard_normal((80, F))
    a = ref.copy()
    a[:, 2000] = ref[:, 2001]
    e = gs.per_row_rel(a, ref, 0)
    assert e.shape == (F,) and e[2000] > 1.0 and np.all(np.delete(e, 2000) == 0.0)
    whole = gs.rms(a, ref) / gs.rms(ref, 0 * ref)
    print("one column of %d misplaced: worst frame %.2f, whole-output rms %.4f" % (F, e[2000], whole))
    assert whole < 0.02
    # rows instead of columns: the encoder's layout
    ref = rng.standard_normal((512, 128))
    a = ref.copy()
    a[300] = ref[299]
    e = gs.per_row_rel(a, ref, 1)
    assert e.shape == (512,) and e[300] > 1.0 and np.all(np.delete(e, 300) == 0.0)
    with pytest.raises(AssertionError):
        gs.per_row_rel(np.zeros((3, 4)), np.zeros((4, 3)), 0)


@pytest.mark.parametrize("F", [37, 100])
def test_a_spoilt_tile_is_a_hundred_bounds_away(orc, orc64, blob, F):
    """One 16-wide K group lost in one 32x32 tile of layer 0, then of layer 4: in the frames of that tile the contribution
    is off by at least 100 x what the GPU test allows at this shape.  (Layer 4 loses a group of the middle tap: the outer
    taps of the first and last two frames multiply the zero padding, and losing a product with zero changes nothing.)"""
    fr, c64, d32 = gs.postnet_ref(orc, orc64, blob, F)
    allowed = gs.bound(d32)
    tm = (F - 1) // 32  # the last row tile (a partial one)
    for spoil in ((0, tm, 3, 7), (0, 0, 15, 24), (4, tm, 2, 95), (4, 0, 0, 64), (4, 0, 1, 80)):
        got = gs.postnet_numpy(orc, blob, fr, spoil=spoil)
        e = gs.per_row_rel(got - fr.T, c64, 0)
        rows = np.arange(32 * spoil[1], min(32 * spoil[1] + 32, F))
        print("spoil %s F=%d: spoilt frames %.2e .. %.2e, bound %.2e, d32 %.2e" % (spoil, F, e[rows].min(), e[rows].max(), allowed, d32))
        assert e[rows].min() >= 100.0 * allowed, (spoil, F, e[rows].min(), allowed)
        if spoil[0] == 4:  # the last layer's error stays in its tile
            assert np.delete(e, rows).max(initial=0.0) <= 1e-12


def test_the_fp32_oracle_is_inside_the_bound_at_every_small_shape(orc, orc64, blob):
    """d32 at every sweep shape of at most 520 rows: finite, far below what a spoilt tile shows (1e-2 and more), so the
    bound 4 d32 + 1e-6 is a statement about rounding only.  The figures are printed: they are the yardsticks of the GPU file."""
    t0 = time.time()
    worst = 0.0
    for F in [F for F in gs.SWEEP_POSTNET if F <= gs.SMALL] + list(gs.FORCED64_POSTNET):
        d32 = gs.postnet_ref(orc, orc64, blob, F)[2]
        print("d32 postnet F=%d: %.2e" % (F, d32))
        worst = max(worst, d32)
    for T, valid in [(T, None) for T in gs.SWEEP_ENCODER] + list(gs.ENCODER_PADDED):
        dm, dp = gs.encoder_ref(orc, orc64, blob, T, valid, synth_ids)[3:]
        print("d32 encoder T=%d valid=%s: memory %.2e processed_memory %.2e" % (T, valid, dm, dp))
        worst = max(worst, dm, dp)
    for F in [F for F in gs.SWEEP_MEL2LIN if F <= gs.SMALL]:
        d32 = gs.mel2lin_ref(orc, orc64, F, 0)[2]
        print("d32 mel2lin F=%d: %.2e" % (F, d32))
        worst = max(worst, d32)
    for F in [F for F in gs.SWEEP_NNLS if F <= gs.SMALL]:
        d32 = gs.mel2lin_ref(orc, orc64, F, gs.NNLS_ITERS)[2]
        print("d32 mel2lin+nnls F=%d: %.2e" % (F, d32))
        worst = max(worst, d32)
    print("worst d32 %.2e in %.1f s" % (worst, time.time() - t0))
    # the fp32 oracle's own error d32 <= 4 d32 + 1e-6 by construction; what has to hold is that the bound stays a rounding-size
    # figure: 2^-24 sqrt(2560) = 3e-6 per GEMM of the longest contraction, a few of them in a row
    assert np.isfinite(worst) and 0.0 < worst <= gs.bound(worst) <= 1e-4, worst
