"""GPU parity of k_gemm_nt at every tile, block mapping, K split and slab loop its callers' row counts select
(tests/gemm_shapes.py restates the plan; test_gemm_shapes_cpu.py shows that these row counts reach every class),
through the public entries: post-net, encoder, mel -> linear with and without the NNLS refinement, the analysis
mel projection, forced 64x64 tiles at small sizes, and the call order on one handle.

The metric looks at one frame (a column of the (80 | 513) x F output) or one encoder row at a time,
|| gpu - f64 || / || f64 ||, and the worst one decides; for the post-net it is taken on the stack's own contribution
out - frames^T, a tenth of the output.  The bound is not the kernel's own figure:

    err(gpu, f64) <= 4 d32 + 1e-6,   d32 = the fp32 oracle's worst per-row distance from the fp64 oracle at that shape

(the factor and the additive term of test_gpu_analysis.py and test_gpu_prosody.py: room for another summation order
and for the device's tanhf / expf / powf differing from glibc's by an ulp or two per cell).  One 16-wide K group lost
in one tile shows as 1e-2 and more in its frames (test_gemm_shapes_cpu.py).
Every case prints its figures ("gemm-shapes ..." lines: pytest -rA shows them for passing tests too)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_shapes as gs
from conftest import synth_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=4, seed=1)
    yield v
    v.close()


@pytest.fixture(scope="module")
def voc_nnls(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=4, seed=1)
    v.set_opts(nnls_iters=gs.NNLS_ITERS)
    yield v
    v.close()


@pytest.mark.parametrize("F", gs.SWEEP_POSTNET)
def test_postnet_sweep(model, orc, orc64, blob, F):
    """model.postnet on standard-normal frames against orc64.postnet, per frame of the stack's contribution.
    Layers 1-3 run 4 / 3 / 2 / 1 K slices (to 256 / 320 / 512 rows), layer 4 four slices to 400 rows and the XCD mapping
    after, all layers the XCD mapping from 2561 and 64x64 tiles from 4033 (layer 4 stays 32x32).
    Measured on an MI355X, err(gpu, f64) | d32 (the test prints them):
      F = 1: 2.82e-07 | 2.76e-07    F = 2: 3.69e-07 | 3.44e-07    F = 15: 5.81e-07 | 3.48e-07    F = 16: 5.55e-07 | 3.87e-07
      F = 17: 6.45e-07 | 3.76e-07    F = 31: 6.36e-07 | 3.69e-07    F = 32: 5.86e-07 | 3.78e-07    F = 33: 6.00e-07 | 4.22e-07
      F = 63: 6.14e-07 | 3.69e-07    F = 64: 6.21e-07 | 4.19e-07    F = 65: 6.88e-07 | 4.12e-07    F = 256: 6.33e-07 | 4.07e-07
      F = 257: 7.05e-07 | 4.46e-07    F = 310: 6.97e-07 | 4.31e-07    F = 320: 7.08e-07 | 4.13e-07    F = 321: 7.65e-07 | 4.03e-07
      F = 400: 7.81e-07 | 4.61e-07    F = 401: 1.17e-06 | 4.24e-07    F = 416: 9.91e-07 | 4.02e-07    F = 481: 1.04e-06 | 4.34e-07
      F = 500: 1.09e-06 | 4.14e-07    F = 512: 1.02e-06 | 4.37e-07    F = 513: 1.22e-06 | 4.16e-07    F = 520: 1.18e-06 | 4.30e-07
      F = 540: 1.17e-06 | 4.42e-07    F = 2560: 1.25e-06 | 4.33e-07    F = 2561: 1.36e-06 | 4.54e-07    F = 4033: 1.21e-06 | 4.29e-07"""
    gs.check_postnet(model, orc, orc64, blob, F)


@pytest.mark.parametrize("T,valid", [(T, None) for T in gs.SWEEP_ENCODER] + list(gs.ENCODER_PADDED))
def test_encoder_sweep(model, orc, orc64, blob, T, valid):
    """model.encoder against orc64.encoder, per row of memory and of processed_memory; with `valid`, that many ids and
    a zero-padded tail.  The convolutions run 4 / 3 / 2 K slices, the BiLSTM projection 2 slices to 256 rows, the memory
    layer 2 slices to 128 rows and the XCD mapping after.
    (With fast_tanh in the cooperative BiLSTM's cell update, 1e-7 absolute on entries of 0.03, every row of memory stood at
    0.94 .. 1.03e-06 whatever the shape and T = 1 at 1.54e-06 against a bound of 1.48e-06: the sweep's one finding, not a GEMM's.
    The cell update now uses fast_tanh_rel, device_utils.h.)
    Measured on an MI355X, memory err(gpu, f64) | d32, processed_memory err(gpu, f64) | d32 (the test prints them):
      T = 1: 1.72e-07 | 1.20e-07, 3.14e-07 | 2.03e-07    T = 5: 1.49e-07 | 1.09e-07, 3.77e-07 | 2.11e-07
      T = 16: 1.46e-07 | 1.10e-07, 3.70e-07 | 2.15e-07    T = 17: 1.40e-07 | 1.20e-07, 3.52e-07 | 2.23e-07
      T = 32: 1.43e-07 | 1.13e-07, 3.98e-07 | 2.20e-07    T = 33: 1.47e-07 | 1.10e-07, 3.77e-07 | 2.36e-07
      T = 100: 1.44e-07 | 1.15e-07, 3.90e-07 | 2.21e-07    T = 128: 1.45e-07 | 1.13e-07, 3.84e-07 | 2.32e-07
      T = 129: 1.45e-07 | 1.14e-07, 5.09e-07 | 2.26e-07    T = 240: 1.46e-07 | 1.12e-07, 5.27e-07 | 2.32e-07
      T = 256: 1.53e-07 | 1.13e-07, 5.61e-07 | 2.24e-07    T = 257: 1.71e-07 | 1.16e-07, 5.85e-07 | 2.27e-07
      T = 310: 1.69e-07 | 1.18e-07, 5.57e-07 | 2.35e-07    T = 320: 1.69e-07 | 1.20e-07, 5.34e-07 | 2.23e-07
      T = 321: 1.77e-07 | 1.14e-07, 5.70e-07 | 2.19e-07    T = 511: 1.82e-07 | 1.21e-07, 5.68e-07 | 2.25e-07
      T = 512: 1.78e-07 | 1.15e-07, 5.55e-07 | 2.31e-07    T = 100 (37 valid): 2.01e-07 | 1.58e-07, 4.03e-07 | 2.60e-07
      T = 321 (37 valid): 2.63e-07 | 1.62e-07, 5.65e-07 | 2.62e-07"""
    ids, m64, p64, dm, dp = gs.encoder_ref(orc, orc64, blob, T, valid, synth_ids)
    mem, pm = model.encoder(ids)
    assert mem.shape == (T, 512) and pm.shape == (T, 128) and np.all(np.isfinite(mem)) and np.all(np.isfinite(pm))
    em, ep = gs.worst(mem, m64, 1), gs.worst(pm, p64, 1)
    print("gemm-shapes encoder        T=%4d valid=%s memory err(gpu,f64) %.2e (row %d) d32 %.2e bound %.2e | processed_memory %.2e (row %d) d32 %.2e bound %.2e  %s" % (
        T, valid, em, int(np.argmax(gs.per_row_rel(mem, m64, 1))), dm, gs.bound(dm), ep, int(np.argmax(gs.per_row_rel(pm, p64, 1))), dp, gs.bound(dp),
        " ".join(gs.shape_class(s, T) for s in gs.ENTRIES["encoder"][0])), flush=True)
    assert em <= gs.bound(dm), (T, valid, em, dm)
    assert ep <= gs.bound(dp), (T, valid, ep, dp)


@pytest.mark.parametrize("F", gs.SWEEP_MEL2LIN)
def test_mel_to_linear_sweep(voc, orc, orc64, F):
    """voc.mel_to_linear (nnls_iters = 0: one GEMM with the powf epilogue, 17 column tiles, the last 1 column wide) against
    orc64.mel_to_linear_opts fed the float32 pinv and basis of the fp32 oracle, per frame.  XCD mapping from 514 rows,
    64x64 tiles from 3585.  Measured on an MI355X, err(gpu, f64) | d32 (the test prints them):
      F = 1: 1.33e-07 | 8.67e-08    F = 16: 1.37e-07 | 9.37e-08    F = 17: 1.44e-07 | 8.83e-08    F = 32: 1.57e-07 | 9.21e-08
      F = 33: 1.50e-07 | 9.19e-08    F = 50: 1.45e-07 | 8.93e-08    F = 513: 1.54e-07 | 1.23e-07    F = 514: 1.56e-07 | 1.05e-07
      F = 520: 3.79e-07 | 2.93e-07    F = 768: 2.70e-07 | 1.14e-07    F = 3584: 2.67e-07 | 1.89e-07    F = 3585: 2.29e-07 | 2.20e-07
      F = 3600: 5.10e-07 | 1.28e-07    F = 544: 1.61e-07 | 1.22e-07    F = 740: 6.84e-07 | 1.40e-07    F = 760: 1.85e-07 | 2.73e-07
      F = 3610: 5.54e-07 | 3.90e-07    F = 3620: 1.07e-06 | 4.40e-07    F = 3640: 7.02e-07 | 3.88e-07    F = 3648: 2.35e-07 | 3.96e-07"""
    gs.check_mel2lin(voc, orc, orc64, F, 0)


@pytest.mark.parametrize("F", gs.SWEEP_NNLS)
def test_mel_to_linear_with_nnls_sweep(voc_nnls, orc, orc64, F):
    """The same with two steps of the NNLS refinement: the residual GEMM (K = 528, beta = -1) under the XCD mapping from 81
    rows, the update GEMM (alpha, the residual before the ReLU) from 529 and on 64x64 tiles from 3585.
    Measured on an MI355X, err(gpu, f64) | d32 (the test prints them):
      F = 1: 1.28e-07 | 9.70e-08    F = 17: 1.50e-07 | 9.27e-08    F = 80: 1.55e-07 | 9.38e-08    F = 81: 1.56e-07 | 9.44e-08
      F = 528: 2.65e-07 | 3.40e-07    F = 529: 1.73e-07 | 1.61e-07    F = 3585: 2.51e-07 | 2.69e-07    F = 64: 1.53e-07 | 1.02e-07
      F = 96: 1.42e-07 | 1.00e-07    F = 240: 1.62e-07 | 1.14e-07    F = 250: 1.87e-07 | 1.61e-07    F = 256: 1.63e-07 | 9.82e-08
      F = 544: 1.79e-07 | 1.39e-07    F = 545: 2.09e-07 | 1.61e-07    F = 740: 3.09e-07 | 1.70e-07    F = 760: 2.33e-07 | 2.24e-07
      F = 768: 2.09e-07 | 3.53e-07    F = 3610: 4.41e-07 | 3.68e-07    F = 3620: 3.14e-07 | 2.45e-07    F = 3640: 2.86e-07 | 2.54e-07
      F = 3648: 5.15e-07 | 4.10e-07"""
    gs.check_mel2lin(voc_nnls, orc, orc64, F, gs.NNLS_ITERS, tag="mel2lin+nnls")


@pytest.mark.parametrize("F", gs.SWEEP_ANALYSIS)
def test_analysis_projection_sweep(voc, orc, orc64, F):
    """voc.analyze(want_S=False) at 256 (F - 1) samples under the rule of test_log_mel_matches_the_fp64_chain (every cell of
    the log-mel, max abs distance, 4 x the float32 restatement's + 1e-6): the projection leaves the plain mapping at 81 rows.
    Measured on an MI355X, max|gpu - f64| | d32 (the test prints them):
      F = 80: 1.60e-05 | 1.77e-05    F = 81: 1.29e-05 | 1.85e-05    F = 88: 1.41e-05 | 1.56e-05    F = 200: 2.20e-05 | 1.46e-05"""
    y, want, d32 = gs.analysis_ref(orc, orc64, F)
    S, mel = voc.analyze(y, want_S=False)
    assert S is None and mel.shape == (80, F) and np.all(np.isfinite(mel))
    dg = float(np.abs(mel - want).max())
    print("gemm-shapes analysis       F=%4d max|gpu-f64| %.2e  d32 %.2e  bound %.2e  %s" % (F, dg, d32, 4.0 * d32 + 1e-6, gs.shape_class("analysis", F)), flush=True)
    assert dg <= 4.0 * d32 + 1e-6, (F, dg, d32)


def test_forced_64x64_tiles_at_small_sizes():
    """XDTTS_GEMM_TILE=64 XDTTS_GEMM_SPLITK=1 (read once per process: a child): the post-net at F = 1, 16, 17, 33, 49, 64, 65, 130
    and mel -> linear at F = 1, 17, 49, 65 on 64x64 tiles -- every fill of the last row tile's four 16-row MFMA tiles -- under
    the same bound, computed in the child.  Measured on an MI355X, err(gpu, f64) | d32 (the child prints them):
      post-net F = 1: 2.95e-07 | 2.76e-07    post-net F = 16: 1.01e-06 | 3.87e-07    post-net F = 17: 1.04e-06 | 3.76e-07
      post-net F = 33: 1.02e-06 | 4.22e-07    post-net F = 49: 1.06e-06 | 4.16e-07    post-net F = 64: 1.06e-06 | 4.19e-07
      post-net F = 65: 1.14e-06 | 4.12e-07    post-net F = 130: 1.09e-06 | 4.09e-07    mel -> linear F = 1: 1.33e-07 | 8.67e-08
      mel -> linear F = 17: 1.44e-07 | 8.83e-08    mel -> linear F = 49: 1.44e-07 | 1.06e-07    mel -> linear F = 65: 1.75e-07 | 9.72e-08"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch\n"
        "import gemm_shapes\n"
        "gemm_shapes.forced_tile_child()\n"
    ) % (root, os.path.join(root, "tests"))
    env = dict(os.environ, XDTTS_GEMM_TILE="64", XDTTS_GEMM_SPLITK="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("gemm-shapes forced64")]
    assert len(lines) == len(gs.FORCED64_POSTNET) + len(gs.FORCED64_MEL2LIN) and all(":t64:" in ln and ":t32:" not in ln for ln in lines), lines
    assert "FORCED64 OK %d" % len(lines) in r.stdout


def test_postnet_call_order_does_not_change_a_bit(pkg, blob):
    """One handle runs the post-net shapes of at most 520 frames in a fixed shuffled order, then in the reverse order: every
    shape returns the same bits both times, and the bits of a fresh handle at F = 37, 257, 401.  Between two calls the
    zero fills of the padded activations are skipped or redone by layout (pp_sig), the split-K workspace and its ticket
    counters are reused across 4 / 3 / 2 / 1 slices, and layer 4 changes from four slices to the XCD mapping and back."""
    m = pkg.Tacotron2.from_blob(blob)
    try:
        first = {F: m.postnet(gs.postnet_frames(F)) for F in gs.ORDER_POSTNET}
        for F in reversed(gs.ORDER_POSTNET):
            again = m.postnet(gs.postnet_frames(F))
            assert np.array_equal(again, first[F]), ("reverse order", F, float(np.abs(again - first[F]).max()))
        # the same shape twice in a row (no fill at all in between), then after a much longer one
        for F in (400, 400, 520, 1, 400):
            assert np.array_equal(m.postnet(gs.postnet_frames(F)), first[F]), ("repeat", F)
    finally:
        m.close()
    for F in gs.FRESH_POSTNET:
        fresh = pkg.Tacotron2.from_blob(blob)
        try:
            out = fresh.postnet(gs.postnet_frames(F))
        finally:
            fresh.close()
        assert np.array_equal(out, first[F]), ("fresh handle", F, float(np.abs(out - first[F]).max()))
    print("gemm-shapes postnet order: %d shapes bit-identical in both orders and on fresh handles" % len(gs.ORDER_POSTNET))


def test_encoder_call_order_does_not_change_a_bit(pkg, blob):
    """The same for the encoder at T = 100, 37, 321, 5, 100 and back (xpad_zero / xpad_B / xpad_T, the workspace and the
    tickets across 4 and 2 slices, the memory layer in and out of the XCD mapping), and fresh handles at T = 37, 321, 100."""
    m = pkg.Tacotron2.from_blob(blob)
    try:
        first = {}
        for T in gs.ORDER_ENCODER:
            out = m.encoder(gs.encoder_ids(T, None, synth_ids))
            if T in first:
                assert np.array_equal(out[0], first[T][0]) and np.array_equal(out[1], first[T][1]), ("second visit", T)
            first[T] = out
        for T in reversed(gs.ORDER_ENCODER):
            mem, pm = m.encoder(gs.encoder_ids(T, None, synth_ids))
            assert np.array_equal(mem, first[T][0]) and np.array_equal(pm, first[T][1]), ("reverse order", T)
        # a zero-padded tail after a full window of the same T: the same layout, so no fill in between
        padded = m.encoder(gs.encoder_ids(100, 37, synth_ids))
        full = m.encoder(gs.encoder_ids(100, None, synth_ids))
        assert np.array_equal(full[0], first[100][0]) and np.array_equal(full[1], first[100][1])
    finally:
        m.close()
    for T in gs.FRESH_ENCODER:
        fresh = pkg.Tacotron2.from_blob(blob)
        try:
            mem, pm = fresh.encoder(gs.encoder_ids(T, None, synth_ids))
            if T == 100:
                p2 = fresh.encoder(gs.encoder_ids(100, 37, synth_ids))
                assert np.array_equal(p2[0], padded[0]) and np.array_equal(p2[1], padded[1]), "padded tail on a fresh handle"
        finally:
            fresh.close()
        assert np.array_equal(mem, first[T][0]) and np.array_equal(pm, first[T][1]), ("fresh handle", T)
    print("gemm-shapes encoder order: T = %s bit-identical in both orders and on fresh handles" % (gs.ORDER_ENCODER,))
