"""Shared by test_gemm_shapes_cpu.py and test_gpu_gemm_shapes.py: the shape plan of k_gemm_nt restated in plain
Python, the call sites that reach it through the public entries, the row counts that reach every shape the
plan produces, the per-row metric, a fp64 numpy post-net that can be spoilt on purpose, and the references
(fp64 oracle, and the fp32 oracle's own distance from it) of every case, computed once.

The rules restated here (csrc/gemm.hip: launch_gemm_nt, gemm_splitk_plan, k_gemm_nt; M = rows of one call):

  tiles64 = ceil(N / 64) ceil(M / 64) batch;  big = N >= 64 and tiles64 >= 512 and not (M <= 128 and N >= 4096)
  xcd     = rows lda > N K                    row tile -> XCD mapping, grid y rounded up to a multiple of 8
  split   (the Tacotron2 handle only, and only when neither big nor xcd):
            sk = min(4, 512 / blocks of 32x32, nslab / 8), nslab = ceil(K / 32);  sk < 2 -> none
            slice ks takes slabs [ks kper, (ks + 1) kper) of kper = ceil(nslab / sk) slabs
  tile    64x64 when big (or the call forces it), else 32x32;  a split call is always 32x32
  slabs   a block runs rounds of 12 unrolled steps while 14 more slabs exist, then the guarded tail of 2 .. 13
"""
import numpy as np

BK = 32                 # csrc/gemm.hip
NBP = 528               # csrc/griffinlim_handle.h: bins padded to the GEMM's K granule
T_MAX = 512             # csrc/common.h: the encoder entry refuses more rows
GEMM_RAGGED_MAX = 64    # csrc/kernels.h
N_MEL, N_BINS, HOP = 80, 513, 256

# call site -> N, K, lda, whether the handle plans split-K (run_gemm), the tile the call forces (0: none)
SITES = {
    "post0": dict(N=512, K=400, lda=80, split=True, tile=0),          # post-net layer 0: 12.5 slabs
    "post13": dict(N=512, K=2560, lda=512, split=True, tile=0),       # post-net layers 1-3
    "post4": dict(N=80, K=2560, lda=512, split=True, tile=0),         # post-net layer 4: transposed store + residual
    "enc_conv": dict(N=512, K=2560, lda=512, split=True, tile=0),     # the three encoder convolutions
    "bilstm_proj": dict(N=1024, K=512, lda=512, split=True, tile=0),  # BiLSTM input projections
    "memory": dict(N=128, K=512, lda=512, split=True, tile=0),        # attention memory layer
    "mel2lin": dict(N=513, K=80, lda=80, split=False, tile=0),        # pinv . exp(mel): 2.5 slabs, last column tile 1 wide
    "nnls_res": dict(N=80, K=NBP, lda=NBP, split=False, tile=0),      # NNLS residual: 16.5 slabs
    "nnls_upd": dict(N=NBP, K=80, lda=80, split=False, tile=0),       # NNLS update
    "analysis": dict(N=80, K=NBP, lda=NBP, split=False, tile=32),     # analysis mel projection
}
# public entry -> the sites one call of it runs, and the row counts it can be given
ENTRIES = {
    "postnet": (("post0", "post13", "post4"), range(1, 4101)),
    "encoder": (("enc_conv", "bilstm_proj", "memory"), range(1, T_MAX + 1)),
    "mel_to_linear": (("mel2lin", "nnls_res", "nnls_upd"), range(1, 3701)),
}

# the sweeps of test_gpu_gemm_shapes.py
# (310, 416, 500, 540 / 240, 310 and the second line of the two vocoder lists are there for the coverage test of
# test_gemm_shapes_cpu.py: the thresholds alone left the classes they reach unswept)
SWEEP_POSTNET = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 256, 257, 310, 320, 321, 400, 401, 416, 481, 500, 512, 513, 520, 540, 2560, 2561, 4033)
SWEEP_ENCODER = (1, 5, 16, 17, 32, 33, 100, 128, 129, 240, 256, 257, 310, 320, 321, 511, 512)
ENCODER_PADDED = ((100, 37), (321, 37))  # (T, valid ids): a zero-padded tail
SWEEP_MEL2LIN = (1, 16, 17, 32, 33, 50, 513, 514, 520, 768, 3584, 3585, 3600,
                 544, 740, 760, 3610, 3620, 3640, 3648)
SWEEP_NNLS = (1, 17, 80, 81, 528, 529, 3585,
              64, 96, 240, 250, 256, 544, 545, 740, 760, 768, 3610, 3620, 3640, 3648)
NNLS_ITERS = 2
SWEEP_ANALYSIS = (80, 81, 88, 200)
FORCED64_POSTNET = (1, 16, 17, 33, 49, 64, 65, 130)
FORCED64_MEL2LIN = (1, 17, 49, 65)
SMALL = 520  # the CPU file computes the references up to here
# call order: the post-net shapes of at most 520 rows in a fixed shuffled order (then reversed), and the encoder's
ORDER_POSTNET = (257, 16, 520, 1, 401, 64, 33, 512, 2, 321, 37, 17, 500, 481, 63, 256, 15, 416, 513, 65, 400, 31, 310, 320, 32)
ORDER_ENCODER = (100, 37, 321, 5, 100)
FRESH_POSTNET = (37, 257, 401)
FRESH_ENCODER = (37, 321, 100)


def cdiv(a, b):
    return -(-a // b)


def plan(site, M, batch=1, force_tile=0, force_nosplit=False):
    """What launch_gemm_nt / gemm_splitk_plan choose for `batch` items of M rows at a call site, or, with M a sequence of
    per-item row counts, for that ragged batch (the post-net's: g.M = the longest item, Mz the items).
    force_tile / force_nosplit: XDTTS_GEMM_TILE / XDTTS_GEMM_SPLITK=1 of the forced-tile child process."""
    return plan_of(SITES[site], M, batch, force_tile, force_nosplit)


def plan_of(s, M, batch=1, force_tile=0, force_nosplit=False):
    """plan() for a site given by its dict (N, K, lda, split, tile) -- vocoder_params.py hands in the vocoder's sites at another
    band count than 80."""
    N, K, lda = s["N"], s["K"], s["lda"]
    Mz = [M] * batch if isinstance(M, (int, np.integer)) else [int(m) for m in M]
    M, batch = max(Mz), len(Mz)
    tiles64 = cdiv(N, 64) * cdiv(M, 64) * batch
    natural_big = N >= 64 and tiles64 >= 512 and not (M <= 128 and N >= 4096)
    rows = sum(Mz)
    xcd = rows * lda > N * K
    nslab = cdiv(K, BK)
    sk = 1
    if s["split"] and not force_nosplit and not natural_big and not xcd:
        blocks = sum(cdiv(m, 32) for m in Mz) * cdiv(N, 32)
        sk = min(4, 512 // max(blocks, 1))
        sk = min(sk, nslab // 8)
        if sk < 2:
            sk = 1
    if sk > 1:
        tile = 32
    elif s["tile"]:
        tile = s["tile"]
    elif force_tile:
        tile = force_tile
    else:
        tile = 64 if natural_big else 32
    kper = cdiv(nslab, sk) * BK
    slabs = tuple(cdiv(min(K - ks * kper, kper), BK) for ks in range(sk))
    row_tiles = sum(cdiv(m, tile) for m in Mz)
    return dict(tile=tile, mapping="xcd" if xcd else "plain", slices=sk, slabs=slabs, row_tiles=row_tiles,
                col_tiles=cdiv(N, tile), padded=bool(xcd and row_tiles % 8 != 0))


def last_row_tile(M, tile):
    """Which waves of the last row tile store: 32x32 has two wave rows of 16, 64x64 two of 32 (2 MFMA tiles each)."""
    rem = M % tile
    if rem == 0:
        return "full"
    if tile == 32:
        return "le16" if rem <= 16 else "gt16"
    return "le16" if rem <= 16 else ("le32" if rem <= 32 else ("le48" if rem <= 48 else "gt48"))


def shape_class(site, M, **kw):
    p = plan(site, M, **kw)
    c = "%s:t%d:%s:s%d:%s:%s" % (site, p["tile"], p["mapping"], p["slices"], "+".join(map(str, p["slabs"])), last_row_tile(M, p["tile"]))
    if p["mapping"] == "xcd":
        c += ":groups-%s" % ("padded" if p["padded"] else "of-8")
    return c


def entry_classes(entry, Ms, sites=None):
    """Every shape class the row counts Ms produce at the sites of an entry (or the named ones of them)."""
    return {shape_class(s, M) for s in (sites or ENTRIES[entry][0]) for M in Ms}


# ---- the metric ------------------------------------------------------------------------------------------------

def per_row_rel(a, ref, axis):
    """|| a - ref ||_2 / || ref ||_2 taken along `axis`, one figure per index of the other axis: per frame of an
    (80 | 513) x F output with axis = 0, per encoder row of a T x C output with axis = 1.  The worst one decides:
    one misplaced row keeps its size here, where an RMS over the whole output dilutes it by sqrt(rows)."""
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape and a.ndim == 2, (a.shape, ref.shape)
    num = np.sqrt(np.sum((a - ref) ** 2, axis=axis))
    den = np.sqrt(np.sum(ref ** 2, axis=axis))
    return num / np.maximum(den, 1e-300)


def worst(a, ref, axis):
    return float(per_row_rel(a, ref, axis).max())


def bound(d32):
    """err(gpu, f64) <= 4 d32 + 1e-6, d32 = the fp32 oracle's worst per-row distance from the fp64 oracle at the shape."""
    return 4.0 * d32 + 1e-6


def rms(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


# ---- fp64 numpy post-net, optionally spoilt ---------------------------------------------------------------------

def postnet_numpy(orc, blob, frames, spoil=None, stale=None):
    """postnet.onnx from the blob's tensors in fp64: 5 x [conv k5 pad 2 + BN(eval)], tanh after the first four, the
    residual added at the end; (80, F).  spoil = (layer, row tile, column tile, K group): that layer's GEMM loses the
    products of one 16-wide group of its contraction index (laid out [tap][channel in], as the kernel's operand is) in
    one 32x32 output tile -- what a slab staged half, or a fragment read from the wrong buffer, would do; with a sequence
    of K groups in place of one, all of them (a whole K slice of a split launch).
    stale = (layer, rows (2, channels in)): that layer reads `rows` where the zero padding behind the last frame should be --
    what a shorter item of a ragged batch reads when the rows up to the longest item's end were not cleared."""
    x = np.asarray(frames, dtype=np.float64)
    F = x.shape[0]
    for i in range(5):
        p = "postnet.convolutions.%d." % i
        w = orc.tensor(blob, p + "conv.weight").astype(np.float64)  # [co][ci][k]
        co, ci, k = w.shape
        pad = (k - 1) // 2
        xp = np.zeros((F + 2 * pad, ci))
        xp[pad:pad + F] = x
        if stale is not None and stale[0] == i:
            xp[pad + F:] = stale[1]
        s = np.zeros((F, co))
        for j in range(k):
            s += xp[j:j + F] @ w[:, :, j].T
        if spoil is not None and spoil[0] == i:
            _, tm, tn, kgs = spoil
            r0, r1, n0, n1 = 32 * tm, min(32 * tm + 32, F), 32 * tn, min(32 * tn + 32, co)
            for kg in (kgs,) if isinstance(kgs, (int, np.integer)) else kgs:
                j, c0 = (16 * kg) // ci, (16 * kg) % ci
                assert r0 < F and n0 < co and j < k, spoil
                s[r0:r1, n0:n1] -= xp[r0 + j:r1 + j, c0:c0 + 16] @ w[n0:n1, c0:c0 + 16, j].T
        s += orc.tensor(blob, p + "conv.bias").astype(np.float64)
        inv = 1.0 / np.sqrt(orc.tensor(blob, p + "bn.running_var").astype(np.float64) + 1e-5)
        s = (s - orc.tensor(blob, p + "bn.running_mean").astype(np.float64)) * inv * orc.tensor(blob, p + "bn.weight").astype(np.float64) \
            + orc.tensor(blob, p + "bn.bias").astype(np.float64)
        x = np.tanh(s) if i < 4 else s
    return (np.asarray(frames, dtype=np.float64) + x).T


# ---- inputs and references, computed once per shape and never modified -------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def postnet_frames(F):
    """(F, 80) standard-normal frames, seeded by F."""
    return np.random.default_rng(F).standard_normal((F, N_MEL)).astype(np.float32)


_POSTNET = {}


def postnet_ref(orc, orc64, blob, F):
    """frames, the fp64 oracle's CONTRIBUTION of the stack (out - frames^T, (80, F)), and d32 on it per frame."""
    if F not in _POSTNET:
        fr = postnet_frames(F)
        c64 = orc64.postnet(blob, fr) - fr.T.astype(np.float64)
        c32 = orc.postnet(blob, fr).astype(np.float64) - fr.T.astype(np.float64)
        _POSTNET[F] = _frozen(fr, c64) + (worst(c32, c64, 0),)
    return _POSTNET[F]


def postnet_err(out, fr, c64):
    """The worst frame of the stack's own contribution of a float32 (80, F) post-net output."""
    return worst(np.asarray(out, dtype=np.float64) - fr.T.astype(np.float64), c64, 0)


def encoder_ids(T, valid=None, synth_ids=None):
    """T ids (seeded by T); with `valid`, that many ids and a zero-padded tail."""
    if valid is None:
        return synth_ids(T, seed=T)
    ids = np.zeros(T, dtype=np.int64)
    ids[:valid] = synth_ids(valid, seed=T)
    return ids


_ENCODER = {}


def encoder_ref(orc, orc64, blob, T, valid, synth_ids):
    """ids, fp64 memory and processed_memory, and d32 per row of each."""
    if (T, valid) not in _ENCODER:
        ids = encoder_ids(T, valid, synth_ids)
        m64, p64 = orc64.encoder(blob, ids)
        m32, p32 = orc.encoder(blob, ids)
        _ENCODER[(T, valid)] = _frozen(ids, m64, p64) + (worst(m32, m64, 1), worst(p32, p64, 1))
    return _ENCODER[(T, valid)]


def mel_input(F):
    """(80, F) natural-log mel of speech-like range, seeded by F (the input of test_mel_to_linear_parity)."""
    return np.random.default_rng(F).uniform(-8, 0.5, size=(N_MEL, F)).astype(np.float32)


_MEL2LIN = {}
_BASIS = {}


def basis_pinv(orc):
    """The float32 mel basis and pseudo-inverse the fp32 oracle produces; both oracles are fed these."""
    if "b" not in _BASIS:
        b = orc.mel_filter_bank()
        _BASIS["b"] = _frozen(b, orc.pinv(b))
    return _BASIS["b"]


def mel2lin_ref(orc, orc64, F, nnls_iters):
    """mel, the fp64 S (513, F), and d32 per frame."""
    if (F, nnls_iters) not in _MEL2LIN:
        basis, pinv = basis_pinv(orc)
        mel = mel_input(F)
        s64 = orc64.mel_to_linear_opts(pinv, basis, mel, power=1.7, nnls_iters=nnls_iters)
        s32 = orc.mel_to_linear_opts(pinv, basis, mel, power=1.7, nnls_iters=nnls_iters)
        _MEL2LIN[(F, nnls_iters)] = _frozen(mel, s64) + (worst(s32, s64, 0),)
    return _MEL2LIN[(F, nnls_iters)]


def chirps(n):
    """Five linear chirps 100 Hz - 7 kHz plus a little noise (the BASELINE config-5 signal), n > 1 samples."""
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(3)
    y = sum(0.15 * np.sin(2 * np.pi * (f0 + 0.5 * (f1 - f0) * t / t[-1]) * t) for f0, f1 in ((100, 900), (400, 2500), (1200, 4000), (3000, 5500), (5000, 7000)))
    return (y + 0.01 * rng.standard_normal(n)).astype(np.float32)


def log_mel_chain(B, m, dtype, floor=1e-5, power=1.7):
    """ln(max(B @ m^power, floor)) in `dtype`: the analysis chain behind the magnitude under the default conventions."""
    mel = B.astype(dtype) @ (m.astype(dtype) ** dtype(power))
    assert mel.dtype == dtype
    return np.log(np.maximum(mel, dtype(floor)))


_ANALYSIS = {}


def analysis_ref(orc, orc64, F):
    """The rule of test_log_mel_matches_the_fp64_chain at n = 256 (F - 1) samples: signal, fp64 log-mel, and d32 =
    the max abs distance of the same chain restated in float32 (fp32 oracle STFT, float32 hypot, ** 1.7, matmul, log)."""
    if F not in _ANALYSIS:
        y = chirps(HOP * (F - 1))
        s64, s32 = orc64.stft(y), orc.stft(y)
        m32 = np.hypot(s32[..., 0], s32[..., 1])
        assert m32.dtype == np.float32 and m32.shape == (N_BINS, F)
        B = orc.mel_filter_bank()
        want = log_mel_chain(B, np.hypot(s64[..., 0], s64[..., 1]), np.float64)
        _ANALYSIS[F] = _frozen(y, want) + (float(np.abs(log_mel_chain(B, m32, np.float32) - want).max()),)
    return _ANALYSIS[F]


# ---- one case each: run, print the error and its yardstick, assert ------------------------------------------------

def check_postnet(model, orc, orc64, blob, F, tag="postnet", **plan_kw):
    fr, c64, d32 = postnet_ref(orc, orc64, blob, F)
    out = model.postnet(fr)
    assert out.shape == (N_MEL, F) and out.dtype == np.float32 and np.all(np.isfinite(out)), (tag, F)
    e = postnet_err(out, fr, c64)
    f = int(np.argmax(per_row_rel(out.astype(np.float64) - fr.T.astype(np.float64), c64, 0)))
    print("gemm-shapes %-14s F=%4d err(gpu,f64) %.2e (frame %d)  d32 %.2e  bound %.2e  %s" % (
        tag, F, e, f, d32, bound(d32), " ".join(shape_class(s, F, **plan_kw) for s in ENTRIES["postnet"][0])), flush=True)
    assert e <= bound(d32), (tag, F, e, d32, f)
    return out


def check_mel2lin(voc, orc, orc64, F, nnls_iters, tag="mel2lin", **plan_kw):
    mel, s64, d32 = mel2lin_ref(orc, orc64, F, nnls_iters)
    S = voc.mel_to_linear(mel)
    assert S.shape == (N_BINS, F) and S.dtype == np.float32 and np.all(np.isfinite(S)), (tag, F)
    e = worst(S, s64, 0)
    sites = ENTRIES["mel_to_linear"][0] if nnls_iters else ("mel2lin",)
    print("gemm-shapes %-14s F=%4d nnls=%d err(gpu,f64) %.2e (frame %d)  d32 %.2e  bound %.2e  %s" % (
        tag, F, nnls_iters, e, int(np.argmax(per_row_rel(S, s64, 0))), d32, bound(d32), " ".join(shape_class(s, F, **plan_kw) for s in sites)), flush=True)
    assert e <= bound(d32), (tag, F, nnls_iters, e, d32)
    return S


def forced_tile_child():
    """The body of the child process of test_forced_64x64_tiles_at_small_sizes (XDTTS_GEMM_TILE=64 XDTTS_GEMM_SPLITK=1 are
    read once per process): the same cases, the same bound, computed here."""
    import importlib

    import oracle

    pkg = importlib.import_module("xd-tts_amd")
    orc, orc64 = oracle.Oracle("f32"), oracle.Oracle("f64")
    blob = orc.weights_synthetic(seed=20240327, rec_scale=1.0)
    kw = dict(force_tile=64, force_nosplit=True)
    m = pkg.Tacotron2.from_blob(blob)
    for F in FORCED64_POSTNET:
        check_postnet(m, orc, orc64, blob, F, tag="forced64", **kw)
    m.close()
    v = pkg.create_griffin_lim(iters=4, seed=1)
    for F in FORCED64_MEL2LIN:
        check_mel2lin(v, orc, orc64, F, 0, tag="forced64", **kw)
    v.close()
    print("FORCED64 OK %d" % (len(FORCED64_POSTNET) + len(FORCED64_MEL2LIN)))
