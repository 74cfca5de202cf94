"""GPU parity of the post-net and of the single-workgroup encoder over the BATCH axis, through the parity hooks postnet_batch and
encoder_batch, which run the code of a batch request: what k_gemm_nt does with several items (split-K across items, the XCD
mapping's row tiles numbered through all items, ragged groups, both stores of the last post-net layer), the post-net's groups of
64 items, and the encoder with the single-workgroup BiLSTM on a (2, B) grid.  tests/batch_shapes.py restates the plans;
test_batch_shapes_cpu.py shows that these batches reach every class.

The other half of the sweep -- the encoder on the handle's own engine, every plan of the cooperative BiLSTM, the call order on one
handle -- is in test_gpu_encoder_batch_shapes.py, on purpose behind test_gpu_bench_line.py in the order of the suite: once a process
has launched a cooperative kernel, a bench.py child of it runs the headline at half its rate (measured on an MI355X: 49 200 ..
50 500 mel-frames/s against 94 000 .. 96 700 behind a parent that has only loaded a model, run the post-net, the single-workgroup
encoder or the vocoder), which is that test's threshold of 50 000.  Nothing in this file launches one.

Every chunk of a batch is compared with its own references: per encoder row of memory and processed_memory, per frame of the
post-net stack's contribution out - frames^T, || gpu - f64 || / || f64 ||, the worst one of the chunk decides, and

    err(gpu, f64) <= 4 d32 + 1e-6,   d32 = the fp32 oracle's worst distance from the fp64 oracle on that same chunk

(the metric and the bound of test_gpu_gemm_shapes.py).  Two chunks swapped, a row tile taken from the neighbouring chunk, an item
one frame off its column offset, stale rows behind a short item or a lost K slice show as 4e-3 and more in the rows they touch,
1 700 bounds and more (test_batch_shapes_cpu.py); the end-to-end batch tests' rms <= 1e-5 over a whole mel passes them.
Every case prints its figures ("batch-shapes ..." lines: pytest -rA shows them for passing tests too) and records them, under
"batch_shapes/...", in the file test_gpu_parity_regimes._report writes."""
import time

import pytest

import batch_shapes as bs
from conftest import synth_ids
from test_gpu_parity_regimes import _report

pytestmark = pytest.mark.gpu


def _record(key, figures):
    _report("batch_shapes/" + key, figures)


@pytest.fixture(scope="module")
def groups(pkg):
    """G of launch_bilstm_coop on this device: CUs / 8, as tacotron2_handle.cpp takes it."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    import torch

    return bs.coop_group(torch.cuda.get_device_properties(pkg.default_device()).multi_processor_count)


@pytest.fixture(scope="module")
def refs(orc, orc64, blob, groups):
    """Every reference of both GPU files, once, on a few threads (the second file finds them cached); the time is printed with
    the first case.  Measured on an MI355X's host: 531 encoder chunks of 13 645 rows and 257 post-net chunks of 6 162 frames in 2.0 s."""
    t0 = time.time()
    ek, pk = bs.encoder_keys(groups), bs.postnet_keys()
    bs.prime(lambda T, k: bs.encoder_ref(orc, orc64, blob, T, k, synth_ids), ek, workers=8)
    bs.prime(lambda F, k: bs.postnet_ref(orc, orc64, blob, F, k), pk, workers=8)
    dt = time.time() - t0
    print("batch-shapes references: %d encoder chunks (%d rows), %d post-net chunks (%d frames): %.1f s on 8 threads" % (
        len(ek), sum(T for T, _ in ek), len(pk), sum(F for F, _ in pk), dt), flush=True)
    _record("reference_seconds", {"seconds": dt, "encoder_rows": sum(T for T, _ in ek), "postnet_frames": sum(F for F, _ in pk)})
    return dt


@pytest.mark.parametrize("name", bs.BILSTM_B)
@pytest.mark.parametrize("T", bs.BILSTM_T)
def test_single_workgroup_bilstm_over_the_batch(model, orc, orc64, blob, refs, groups, T, name):
    """encoder_batch with the single-workgroup recurrence chosen directly (a request reaches it with several chunks only after a
    timed-out exchange): k_bilstm on a (2, B) grid at T = 1, 2, 3, 5, 17 and the batch sizes of the cooperative sweep, B = 2, G,
    G + 1, 2 G - 1, 52, 2 G, 2 G + 1, 2 G + 2 (G = CUs / 8 = 32), every chunk and every row.
    Measured on an MI355X, the chunk closest to its bound over the 40 cases, err(gpu, f64) | d32 | bound:
      memory 2.83e-07 | 1.25e-07 | 1.50e-06 (B = 63, T = 17)   processed_memory 6.83e-07 | 2.00e-07 | 1.80e-06 (B = 63, T = 3)
    and no case took more than 1 ms."""
    B, _ = bs.bilstm_batches(groups)[name]
    bs.check_encoder(model, orc, orc64, blob, synth_ids, B, T, "single", _record, "bilstm", {"grid-2xB", bs.exchange_class(T)})


@pytest.mark.parametrize("name", list(bs.POSTNET_CASES))
def test_postnet_batch_sweep(model, orc, orc64, blob, refs, name):
    """postnet_batch on a list of chunks in both layouts: the (80 x sum F) matrix and the dense matrices per chunk are equal bit
    for bit, and every frame of every chunk is within its chunk's bound.  The lists: layers 1-3 at 4 / 3 / 2 / 1 slices with items
    that end before the longest, layer 4 either side of 400 frames and layers 0-3 either side of 2560 at 50 items (32x32) and 64
    items (64x64), groups of 8 row tiles full and padded with one-frame items among them, 64 items of which one or two are long
    (layer 4 on 64x64 tiles that hold one to three rows), the same items in two orders, and 64 / 65 / 66 / 130 items (one, two
    and three groups of GEMM_RAGGED_MAX).
    The sweep found no frame outside its bound and no bit of difference between the layouts.  Measured on an MI355X, the chunk
    closest to its bound per list, err(gpu, f64) | d32 (the test prints them; both layouts of a list take 0 .. 4 ms):
      pair: 5.99e-07 | 3.57e-07                  five: 6.22e-07 | 3.71e-07                  five-longest-first: 6.22e-07 | 3.71e-07
      tiles10-s3: 7.14e-07 | 3.87e-07            tiles12-s2: 8.06e-07 | 3.78e-07            tiles13-s2: 8.03e-07 | 4.17e-07
      tiles17-s1: 9.16e-07 | 3.75e-07            sum400: 8.03e-07 | 4.17e-07                sum401: 1.01e-06 | 3.87e-07
      sum438-short: 1.12e-06 | 3.87e-07          n51-post4-s3: 9.40e-07 | 3.66e-07          n50-sum2560: 1.20e-06 | 3.78e-07
      n50-sum2561: 1.20e-06 | 3.78e-07           n52-sum2613: 1.20e-06 | 3.78e-07           n53-sum2620: 1.20e-06 | 3.78e-07
      n64-sum2560: 1.17e-06 | 3.72e-07           n64-sum2561: 1.17e-06 | 3.72e-07           n64-sum2620: 1.17e-06 | 3.72e-07
      n64-one-long: 1.13e-06 | 4.23e-07          n64-two-long-sum417: 1.12e-06 | 3.87e-07   n64-one-long-shuffled: 1.13e-06 | 4.23e-07
      n64: 1.01e-06 | 3.75e-07                   n65: 1.01e-06 | 3.75e-07                   n66: 1.01e-06 | 3.75e-07
      n130: 1.01e-06 | 3.75e-07"""
    bs.check_postnet(model, orc, orc64, blob, name, _record)
