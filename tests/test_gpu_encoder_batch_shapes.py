"""GPU parity of the encoder over the BATCH axis on the engines a batch request uses: the three GEMM sites with B items (split-K
across items, the XCD mapping's row tiles numbered through all items), every plan of the cooperative BiLSTM (one or two chunks per
group of workgroups, several launches over one exchange buffer), and the call order of encoder batches and post-net lists on one
handle.  The post-net's lists and the single-workgroup BiLSTM are in test_gpu_batch_shapes.py, which also says why this half stands
in a file of its own: it launches cooperative kernels, and must not do so in front of test_gpu_bench_line.py.
The metric, the bound, the helper and the CPU file are those of test_gpu_batch_shapes.py."""
import numpy as np
import pytest

import batch_shapes as bs
from conftest import synth_ids
from test_gpu_batch_shapes import _record, groups, refs  # noqa: F401  (the fixtures of the first half)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,T", bs.ENCODER_CASES)
def test_encoder_batch_sweep(model, orc, orc64, blob, refs, B, T):
    """encoder_batch (the handle's own BiLSTM engine: the cooperative one) on the first B chunks of window T's pool, every third
    with a zero-padded tail, every chunk and every row against the chunk's own fp64 reference.  The batches reach all 20 (site,
    tile, mapping, slices, fill of the last group) plans a batch of at most 66 chunks of at most 128 ids gives the three encoder
    GEMM sites, with split-K across items, item boundaries inside a group of 8 row tiles and chunks of less than one tile.
    The sweep found no chunk outside its bound.  Measured on an MI355X, the chunk closest to its bound per case, memory
    err(gpu, f64) | d32, processed_memory err(gpu, f64) | d32 (the test prints them; each case takes 0 .. 2 ms on the GPU):
      (2, 1): 1.62e-07 | 1.19e-07, 3.59e-07 | 2.14e-07      (9, 1): 2.15e-07 | 1.18e-07, 3.89e-07 | 2.10e-07
      (11, 1): 2.16e-07 | 1.16e-07, 3.91e-07 | 2.01e-07     (17, 1): 2.15e-07 | 1.18e-07, 4.07e-07 | 1.93e-07
      (65, 1): 2.22e-07 | 1.10e-07, 5.26e-07 | 1.96e-07     (33, 1): 2.22e-07 | 1.10e-07, 4.07e-07 | 1.93e-07
      (2, 65): 1.48e-07 | 1.13e-07, 5.67e-07 | 2.32e-07     (4, 33): 1.81e-07 | 1.27e-07, 5.80e-07 | 2.26e-07
      (61, 17): 2.71e-07 | 1.25e-07, 6.28e-07 | 2.20e-07    (16, 65): 3.09e-07 | 1.52e-07, 6.12e-07 | 2.38e-07
      (22, 48): 3.01e-07 | 1.41e-07, 6.39e-07 | 2.28e-07    (24, 48): 3.01e-07 | 1.41e-07, 6.39e-07 | 2.28e-07
      (41, 63): 3.07e-07 | 1.41e-07, 6.22e-07 | 2.36e-07    (26, 100): 2.97e-07 | 1.36e-07, 6.18e-07 | 2.15e-07
      (40, 65): 2.99e-07 | 1.38e-07, 5.94e-07 | 2.20e-07    (41, 65): 2.99e-07 | 1.38e-07, 5.94e-07 | 2.20e-07
      (64, 41): 3.01e-07 | 1.35e-07, 6.01e-07 | 2.22e-07    (65, 41): 3.01e-07 | 1.35e-07, 6.01e-07 | 2.22e-07
      (8, 17): 1.52e-07 | 1.09e-07, 5.68e-07 | 2.24e-07
    The slowest case of the two GPU files is the call-order test, 1.2 s."""
    bs.check_encoder(model, orc, orc64, blob, synth_ids, B, T, None, _record, "encoder", bs.encoder_classes(B, T))


@pytest.mark.parametrize("name", bs.BILSTM_B)
@pytest.mark.parametrize("T", bs.BILSTM_T)
def test_cooperative_bilstm_plans(model, orc, orc64, blob, refs, groups, T, name):
    """The cooperative recurrence at T = 1 (no exchange), 2 (one), 3 (both parity slots), 5 and 17, for B = 2, G, G + 1, 2 G - 1,
    52, 2 G, 2 G + 1, 2 G + 2 chunks (G = CUs / 8 = 32): one chunk per group, two per group with a last group of one or two, a
    second launch of one or two chunks over the re-zeroed exchange buffer.  The class each B is there for is asserted.
    Measured on an MI355X (G = 32), the chunk closest to its bound over the 40 cases, err(gpu, f64) | d32 | bound:
      memory 2.71e-07 | 1.25e-07 | 1.50e-06 (B = 63, T = 17)   processed_memory 6.63e-07 | 2.00e-07 | 1.80e-06 (B = 63, T = 3)
    and no case took more than 1 ms."""
    B, want = bs.bilstm_batches(groups)[name]
    cls = bs.bilstm_class(B, groups)
    assert cls == want, (name, B, groups, cls, want)
    bs.check_encoder(model, orc, orc64, blob, synth_ids, B, T, "cooperative", _record, "bilstm", {cls, bs.exchange_class(T)})


def _run(m, op):
    if op[0] == "enc":
        ids = np.stack([bs.encoder_chunk(op[2], k, synth_ids) for k in range(op[1])])
        return m.encoder_batch(ids, engine=op[3])
    if op[0] == "enc1":
        return m.encoder(bs.encoder_chunk(op[1], 0, synth_ids))
    if op[0] == "post1":
        return (m.postnet(bs.postnet_chunk(op[1], 0)),)
    out = m.postnet_batch([bs.postnet_chunk(F, k) for F, k in bs.list_items(bs.postnet_list(op[1]))], per_chunk=op[2])
    return tuple(out) if op[2] else (out,)


def test_call_order_does_not_change_a_bit(pkg, blob):
    """A fixed shuffled sequence of encoder batches, post-net lists and the single-chunk hooks on ONE handle: each result equals,
    bit for bit, the same call on a fresh handle.  In between the zero fills are skipped or redone by layout (xpad_B / xpad_T,
    pp_sig), the split-K workspace and tickets are reused across other item counts, the exchange buffer across other plans; a list
    of shorter items follows straight on a longer one of the same n and Fmax, a smaller B on a larger one at the same T."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    fresh = {}
    for op in bs.ORDER:
        if op not in fresh:
            h = pkg.Tacotron2.from_blob(blob)
            try:
                fresh[op] = _run(h, op)
            finally:
                h.close()
    m = pkg.Tacotron2.from_blob(blob)
    try:
        for rnd in range(2):  # the second round starts from the state the first one left
            for i, op in enumerate(bs.ORDER):
                got = _run(m, op)
                assert len(got) == len(fresh[op])
                for j, (a, b) in enumerate(zip(got, fresh[op])):
                    assert a.shape == b.shape and np.array_equal(a, b), (rnd, i, op, j, float(np.abs(a - b).max()))
    finally:
        m.close()
    print("batch-shapes call order: %d calls twice over on one handle, each bit-identical to a fresh handle's" % len(bs.ORDER))
