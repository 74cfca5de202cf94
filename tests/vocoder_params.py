"""Shared by test_vocoder_params_cpu.py and test_gpu_vocoder_params.py: the grid of constructor parameters
xdtts_griffinlim_new accepts (mel basis, power, momentum, iteration count), the rules of k_gemm_nt that move with the
basis restated in plain Python, and the references (fp64 oracle, and the fp32 oracle's own distance from it) of every
case, computed once.

The rules restated here (csrc/gemm.hip: k_gemm_nt's GEMM_FETCH / GEMM_STAGE, launch_gemm_nt; csrc/griffinlim_handle.cpp):

  slabs   K = n_mels columns make ceil(K / 32) slabs of the mel -> linear and NNLS update GEMMs; K % 32 = 16 leaves the last
          one half full.  The pipeline's prologue fetches slabs 0 .. 5 whatever the count, the rounds up to slab nslab + 5.
  fetch   thread tid loads 4 columns per row and slab, lc = (tid & 7) * 4 into the slab.  A slice of a split launch owns columns
          [kbeg, kbeg + KL), kper = ceil(nslab / slices) * 32, kbeg = slice * kper, KL = min(K - kbeg, kper).  A lane whose
          columns slab * 32 + lc .. + 3 lie inside the slice loads them; every other lane is masked by GEMM_STAGE and loads its
          columns of slab 0, k0_ = 0.  The lane's base holds lcs = lc < KL ? lc : 0 in place of lc: with KL = 16 the lanes with
          lc >= 16 have no column in any slab and load columns kbeg .. kbeg + 3.  The rule before this file was written had lc in
          the base: columns kbeg + lc .. + 3 for a masked lane, past the row at K = 16 (fetch_parent below, kept for the test
          that shows the check bites).
  xcd     rows * lda > N * K turns the row-tile-per-XCD mapping on.  For the analysis projection and the NNLS residual
          (N = n_mels, K = lda = 528) that is rows > n_mels: the flip moves with the basis.
"""
import numpy as np

import gemm_shapes as gs
import gl_shapes as gl

BK = gs.BK
N_BINS, HOP, NBP = gs.N_BINS, gs.HOP, gs.NBP
NOVERLAP = 1024 - HOP

# ---- the grid ----------------------------------------------------------------------------------------------------
# name -> (n_mels, fmax): orc.mel_filter_bank(n_mels=..., fmax=...) at 22 050 Hz, n_fft 1024, fmin 0
BASES = {
    "m16": (16, 8000.0), "m32": (32, 8000.0), "m48": (48, 8000.0), "m64": (64, 8000.0), "m80": (80, 8000.0),  # m80: the control
    "m96": (96, 8000.0), "m112": (112, 8000.0), "m128": (128, 8000.0),
    "m128w": (128, 11025.0),  # a second filter-bank geometry
}
RANK_DEFICIENT = (160, 11025.0)  # more bands than the 1024-point grid resolves at the low end: an error case
POWERS = (1.0, 1.7, 2.0, 0.6)    # 1.0: the exponent-free epilogue of the GEMM
MOMENTA = (0.0, 0.5, 0.99)
ITERS = (0, 1, 2)                # given to the constructor: the only route to 0 (infer_linear(iters=0) = the handle's count)
SEED = 3
HOP_REF_MAX = 6e-5               # the fp32 oracle's worst hop against fp64 a loop case may show (check_audio's 1e-3 = 17 x that)

# the sweeps of test_gpu_vocoder_params.py
MEL2LIN_F = (1, 31, 33, 70)
MEL2LIN_POWER_BASES = ("m16", "m48", "m80")
MEL2LIN_POWER_F = (1, 33)
MEL2LIN_XCD = (("m16", 520), ("m128", 520))  # F > 513: the row-tile-per-XCD mapping of pinv . exp(mel)
NNLS_BASES = ("m16", "m48", "m128")
NNLS_MODES = ((1, 0), (7, 0), (0, 1), (0, 2), (7, 1))  # (nnls_iters, power_mode)
ANALYSIS_BASES = ("m16", "m80", "m128")
LOOP_F = (10, 17, 40)            # launch-per-iteration, persistent, persistent
LOOP_MOMENTA = (0.0, 0.5)
E2E_F = 40
E2E_ITERS = 2
BATCH_BASES = ("m16", "m128")
BATCH_F = (2, 17, 40)


def n_mels_of(key):
    return BASES[key][0]


def nnls_frames(key):
    """F on both sides of the NNLS residual's flip rows > n_mels."""
    n = n_mels_of(key)
    return (n - 7, n + 13)


def analysis_frames(key):
    """F on both sides of the analysis projection's flip rows > n_mels."""
    n = n_mels_of(key)
    return (n, n + 1)


# ---- k_gemm_nt restated: slabs, fetch, the flip ---------------------------------------------------------------------

def nslab(K):
    return gs.cdiv(K, BK)


def slab_class(K):
    """K in slabs: 0.5, 1, 1.5, ... (the prologue's guarded cases are 1 and 2 slabs; 3 and more enter the rounds)."""
    assert K % 16 == 0 and K > 0
    return K / BK


def slices_possible(K):
    """Every slice count gemm_splitk_plan can return for a K: 1, and 2 .. min(4, nslab / 8)."""
    return range(1, max(1, min(4, nslab(K) // 8)) + 1)


def slice_range(K, sk, ks):
    """(kbeg, KL) of slice ks of sk (k_gemm_nt; gemm_shapes.plan's slabs are ceil(KL / 32))."""
    kper = gs.cdiv(nslab(K), sk) * BK
    kbeg = ks * kper
    return kbeg, min(K - kbeg, kper)


def fetch(K, sk, ks, slab, tid):
    """The first of the four columns of its row that thread tid loads for `slab` of its slice, and whether GEMM_STAGE
    keeps the value."""
    kbeg, KL = slice_range(K, sk, ks)
    lc = (tid & 7) * 4
    lcs = lc if lc < KL else 0
    ok = slab < gs.cdiv(KL, BK) and slab * BK + lc < KL
    k0 = slab * BK if ok else 0
    return kbeg + lcs + k0, ok


def fetch_parent(K, sk, ks, slab, tid):
    """The same under the rule the kernel had before: lc itself in the lane's base."""
    kbeg, KL = slice_range(K, sk, ks)
    lc = (tid & 7) * 4
    ok = slab < gs.cdiv(KL, BK) and slab * BK + lc < KL
    k0 = slab * BK if ok else 0
    return kbeg + lc + k0, ok


def fetched_slabs(K, sk, ks):
    """The slab indices a block asks GEMM_FETCH for: the prologue's 0 .. 5 and, from the rounds, up to 6 past the last step."""
    return range(0, gs.cdiv(slice_range(K, sk, ks)[1], BK) + 6)


def fetch_violations(K, rule=fetch):
    """Every (slices, slice, slab, tid, first column) at which `rule` forms an address outside columns [0, K) of the row,
    and a check that the kept loads are exactly the columns of the slice, each once."""
    bad = []
    for sk in slices_possible(K):
        kept = []
        for ks in range(sk):
            kbeg, KL = slice_range(K, sk, ks)
            assert KL > 0 and KL % 16 == 0, (K, sk, ks, KL)
            for slab in fetched_slabs(K, sk, ks):
                for tid in range(8):  # (tid & 7 decides; tid >> 3 picks the row)
                    c, ok = rule(K, sk, ks, slab, tid)
                    if c < 0 or c + 3 >= K:
                        bad.append((sk, ks, slab, tid, c))
                    if ok:
                        kept.extend(range(c, c + 4))
        assert sorted(kept) == list(range(K)), (K, sk)
    return bad


def sites(key):
    """The vocoder's four GEMM call sites (gemm_shapes.SITES) at a basis of the grid."""
    n = n_mels_of(key)
    return {
        "mel2lin": dict(N=N_BINS, K=n, lda=n, split=False, tile=0),
        "nnls_res": dict(N=n, K=NBP, lda=NBP, split=False, tile=0),
        "nnls_upd": dict(N=NBP, K=n, lda=n, split=False, tile=0),
        "analysis": dict(N=n, K=NBP, lda=NBP, split=False, tile=32),
    }


def plan(key, site, M):
    return gs.plan_of(sites(key)[site], M)


def analysis_xcd(key, rows):
    """The xcd_rows flip of the analysis projection (and of the NNLS residual): rows * 528 > n_mels * 528."""
    return rows > n_mels_of(key)


def shape_class(key, site, M):
    p = plan(key, site, M)
    return "%s/%s:t%d:%s:%s:%s" % (key, site, p["tile"], p["mapping"], "+".join(map(str, p["slabs"])), gs.last_row_tile(M, p["tile"]))


# ---- inputs and references, computed once per case and never modified -----------------------------------------------

_BASIS = {}


def basis_pinv(orc, key):
    """The float32 basis and pseudo-inverse the fp32 oracle produces; both oracles are fed these."""
    if key not in _BASIS:
        n, fmax = BASES[key]
        b = orc.mel_filter_bank(n_mels=n, fmax=fmax)
        _BASIS[key] = gs._frozen(b, orc.pinv(b))
    return _BASIS[key]


def rank_deficient_basis(orc):
    n, fmax = RANK_DEFICIENT
    return orc.mel_filter_bank(n_mels=n, fmax=fmax)


def mel_input(key, F):
    """(n_mels, F) natural-log mel of speech-like range (gemm_shapes.mel_input's), seeded by the band count and F."""
    n = n_mels_of(key)
    return np.random.default_rng([n, F, len(key)]).uniform(-8, 0.5, size=(n, F)).astype(np.float32)


def speech_mel(key, F):
    """(n_mels, F) natural-log mel for the end-to-end cases (gl_shapes.speech_mel's)."""
    n = n_mels_of(key)
    rng = np.random.default_rng([n, F, 7, len(key)])
    return (rng.uniform(-7.0, -1.0, size=(n, F)) + 1.5 * np.sin(np.arange(F) / 6.0)[None, :]).astype(np.float32)


_MEL2LIN = {}


def mel2lin_ref(orc, orc64, key, F, power=1.7, nnls_iters=0, power_mode=0):
    """mel, the fp64 S (513, F), and d32 per frame."""
    k = (key, F, power, nnls_iters, power_mode)
    if k not in _MEL2LIN:
        basis, pinv = basis_pinv(orc, key)
        mel = mel_input(key, F)
        kw = dict(power=power, nnls_iters=nnls_iters, power_mode=power_mode)
        s64 = orc64.mel_to_linear_opts(pinv, basis, mel, **kw)
        s32 = orc.mel_to_linear_opts(pinv, basis, mel, **kw)
        _MEL2LIN[k] = gs._frozen(mel, s64) + (gs.worst(s32, s64, 0),)
    return _MEL2LIN[k]


_ANALYSIS = {}


def analysis_ref(orc, orc64, key, F, power=1.7):
    """gemm_shapes.analysis_ref at a basis and a power: the chirp signal of 256 (F - 1) samples, the fp64 log-mel, d32 = the
    max abs distance of the chain restated in float32, the fp64 magnitude and the fp32 oracle's."""
    k = (key, F, power)
    if k not in _ANALYSIS:
        y = gs.chirps(HOP * (F - 1))
        s64, s32 = orc64.stft(y), orc.stft(y)
        m64 = np.hypot(s64[..., 0], s64[..., 1])
        m32 = np.hypot(s32[..., 0], s32[..., 1])
        assert m32.dtype == np.float32 and m32.shape == (N_BINS, F)
        B = basis_pinv(orc, key)[0]
        want = gs.log_mel_chain(B, m64, np.float64, power=power)
        d32 = float(np.abs(gs.log_mel_chain(B, m32, np.float32, power=power) - want).max())
        _ANALYSIS[k] = gs._frozen(y, want) + (d32,) + gs._frozen(m64, m32)
    return _ANALYSIS[k]


_LOOP = {}


def loop_ref(orc, orc64, F, momentum, iters):
    """S (the chirp magnitude), phase0 and the two oracles' audio after `iters` iterations at `momentum` (0 iterations: the
    inverse STFT of S e^{i phase0}, which the oracle's loop gives too)."""
    k = (F, momentum, iters)
    if k not in _LOOP:
        S = gl.chirp_S(orc, F)
        p0 = orc.phase_init(SEED, N_BINS, F)
        f32 = orc.griffinlim(S, phase0=p0, iters=iters, momentum=momentum)
        f64 = orc64.griffinlim(S, phase0=p0, iters=iters, momentum=momentum)
        _LOOP[k] = gs._frozen(S, p0, f32, f64)
    return _LOOP[k]


def istft_of_start(orc64, S, p0):
    """orc64.istft of S e^{i phase0}: what 0 iterations deliver, without the oracle's loop."""
    return orc64.istft(np.asarray(S, dtype=np.float64)[..., None] * np.asarray(p0, dtype=np.float64))


_STEP = {}


def step_ref(orc, orc64, F, momentum):
    """The fp32 oracle's state two iterations in (momentum term live), and both oracles' state one iteration later."""
    k = (F, momentum)
    if k not in _STEP:
        S, p0 = loop_ref(orc, orc64, F, momentum, 2)[:2]
        a, r = orc.griffinlim_step(S, p0, np.zeros_like(p0), iters=2, momentum=momentum)
        o32 = orc.griffinlim_step(S, a, r, iters=1, momentum=momentum)
        o64 = orc64.griffinlim_step(S, a, r, iters=1, momentum=momentum)
        _STEP[k] = (S,) + gs._frozen(a, r) + (gs._frozen(*o32), gs._frozen(*o64))
    return _STEP[k]


_E2E = {}


def e2e_ref(orc, orc64, key, F, power=1.7, momentum=0.99):
    """The mel, and both oracles' audio after E2E_ITERS iterations from orc.phase_init(SEED, 513, F) on the fp32 oracle's own
    mel -> linear (as test_gpu_griffinlim_shapes.batch_ref does)."""
    k = (key, F, power, momentum)
    if k not in _E2E:
        pinv = basis_pinv(orc, key)[1]
        mel = speech_mel(key, F)
        S = orc.mel_to_linear(pinv, mel, power=power)
        p0 = orc.phase_init(SEED, N_BINS, F)
        f32 = orc.griffinlim(S, phase0=p0, iters=E2E_ITERS, momentum=momentum)
        f64 = orc64.griffinlim(S, phase0=p0, iters=E2E_ITERS, momentum=momentum)
        _E2E[k] = gs._frozen(mel, f32, f64)
    return _E2E[k]


def audio_figures(a, f32, f64):
    """(rms gpu-f64, rms f32-f64, rms gpu-f32, worst hop gpu-f64, worst hop f32-f64)"""
    return gl.rms(a, f64), gl.rms(f32, f64), gl.rms(a, f32), gl.worst_hop(a, f64), gl.worst_hop(f32, f64)
