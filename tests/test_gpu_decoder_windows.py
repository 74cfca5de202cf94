"""GPU parity of every decoder engine over the encoder window T (1..512; 1..128 on the persistent kernels) and over the
n_valid of each chunk (tests/decoder_windows.py restates what the engines do with T; test_decoder_windows_cpu.py shows that
these windows reach every class of it), through the parity hook decoder_steps and through the public batch entry.

Every chunk starts from a crafted state -- a non-uniform previous alignment with extra weight on the first and last valid
position and on both sides of every class edge, LSTM vectors of N(0, 0.3) -- and every output is compared with the fp64
oracle's step from the same state.  The alignment is compared position by position, max |gpu[t] / f64[t] - 1| over t < n_valid
(t >= n_valid: exactly 0), the other eight outputs as max |gpu - f64| / max(1, |f64|_inf), each chunk on its own.  The bound is
not the kernels' own figure:

    err(gpu, f64) <= 4 d32 + 1e-6,   d32 = the fp32 oracle's distance from the fp64 oracle in the same metric at the same case

(the factor and the additive term of test_gpu_gemm_shapes.py, test_gpu_analysis.py and test_gpu_prosody.py).  One window element
lost shows as 4.7e-04 .. 1.5e-02 on the alignment ratio, 145 bounds and more (test_decoder_windows_cpu.py); the engine tests'
1e-5 absolute on the frame passes it from T = 128 on.
Every case prints its figures ("decoder-windows ..." lines: pytest -rA shows them for passing tests too) and records them, under
"decoder_windows/...", in the file test_gpu_parity_regimes._report writes (those entries are committed as profiles/decoder_windows.json)."""
import os

import numpy as np
import pytest

import decoder_windows as dw
from conftest import synth_ids
from gemm_shapes import bound as frame_bound
from gemm_shapes import per_row_rel
from test_gpu_parity_regimes import _report

pytestmark = pytest.mark.gpu

CASES = [(e, B, T) for e, B in dw.ENGINES for T in sorted(dw.SWEEPS[e])]  # smallest windows first
CASES3 = [(e, B, T) for e, B in dw.ENGINES for T in sorted(dw.STEPS3[e])]


def _record(key, figures):
    _report("decoder_windows/" + key, figures)


def _opts(pkg):
    return pkg.default_opts(dropout_seed=dw.DROPOUT_SEED, item_base=dw.ITEM_BASE)


@pytest.mark.parametrize("engine,B,T", CASES)
def test_one_step_from_a_crafted_state(pkg, model, orc, orc64, blob, engine, B, T):
    """One decoder_iter call per engine, batch size and window from step 4, and from step 5 at a third of the windows (the other
    dropout counter, the other ping-pong half): all nine outputs, chunk by chunk.  The location features of this step come from
    the hook's prologue (batched, launch) or the kernel's set-up (persistent).
    The sweep found no window outside the bound.  Measured on an MI355X, the chunk closest to its bound per engine,
    err(gpu, f64) | d32 | bound (the test prints every case):
      persistent   alignment 2.12e-07 | 1.51e-07 | 1.60e-06 (B = 2, T = 64)            rest 1.68e-07 | 1.07e-07 | 1.43e-06 (attention_cell, B = 2, T = 16)
      persistent8  alignment 2.14e-07 | 7.04e-08 | 1.28e-06 (B = 16, T = 15)           rest 3.98e-07 | 7.61e-08 | 1.30e-06 (decoder_cell, B = 16, T = 63)
      launch       alignment 2.23e-07 | 2.17e-07 | 1.87e-06 (B = 3, T = 112)           rest 1.41e-07 | 5.89e-08 | 1.24e-06 (decoder_output, B = 3, T = 1)
      batched      alignment 2.60e-07 | 1.69e-07 | 1.68e-06 (B = 17, T = 64, step 5)   rest 2.80e-07 | 9.95e-08 | 1.40e-06 (decoder_cell, B = 17, T = 512)"""
    for step0 in (dw.STEP0, dw.STEP0 + 1) if dw.second_step0(T) else (dw.STEP0,):
        dw.check_case(model, _opts(pkg), orc, orc64, blob, engine, B, T, step0, 1, _record, tag="one")


@pytest.mark.parametrize("engine,B,T", CASES3)
def test_three_steps_from_a_crafted_state(pkg, model, orc, orc64, blob, engine, B, T):
    """Three steps from the same states: the second and third take their location features from inside the loop -- the batched
    engine's location blocks riding in the prenet launch (awc / awc2 by parity), the persistent kernels' own location role.  Every
    frame, every gate logit and the seven written-back tensors against three oracle steps per precision.
    Measured on an MI355X, the chunk closest to its bound per engine, err(gpu, f64) | d32 | bound:
      persistent   alignment 1.96e-07 | 1.46e-07 | 1.59e-06 (B = 1, T = 64)     rest 1.45e-07 | 5.61e-08 | 1.22e-06 (attention_hidden, B = 2, T = 64)
      persistent8  alignment 1.95e-07 | 1.22e-07 | 1.49e-06 (B = 16, T = 16)    rest 2.73e-07 | 1.05e-07 | 1.42e-06 (attention_cell, B = 16, T = 128)
      launch       alignment 2.43e-07 | 2.60e-07 | 2.04e-06 (B = 3, T = 100)    rest 1.24e-07 | 9.27e-08 | 1.37e-06 (decoder_output, B = 3, T = 65)
      batched      alignment 3.16e-07 | 1.79e-07 | 1.72e-06 (B = 17, T = 128)   rest 3.26e-07 | 1.05e-07 | 1.42e-06 (attention_cell, B = 17, T = 193)"""
    dw.check_case(model, _opts(pkg), orc, orc64, blob, engine, B, T, dw.STEP0, 3, _record, tag="three")


FORMS = {"fused0": dict(XDTTS_ATT_FUSED="0"), "fused1": dict(XDTTS_ATT_FUSED="1"), "fused2": dict(XDTTS_ATT_FUSED="2"), "notail": dict(XDTTS_NO_TAIL="1")}
PLAN_KW = {"fused0": dict(att_fused=0), "fused1": dict(att_fused=1), "fused2": dict(), "notail": dict(no_tail=True)}


@pytest.fixture(scope="module")
def form_handles(pkg, blob):
    """One handle per attention form of the batched engine; the variables are read when a handle is created."""
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    hs = {}
    for name, var in FORMS.items():
        os.environ.update(var)
        try:
            hs[name] = pkg.Tacotron2.from_blob(blob)
        finally:
            for k in var:
                del os.environ[k]
    yield hs
    for h in hs.values():
        h.close()


@pytest.mark.parametrize("T", dw.FORMS_T)
@pytest.mark.parametrize("B", [6, 17])
@pytest.mark.parametrize("form", list(FORMS))
def test_batched_attention_forms_over_the_window(pkg, form_handles, orc, orc64, blob, form, B, T):
    """The batched engine's attention as two kernels (XDTTS_ATT_FUSED=0: k_softmax_ctx, 256 threads), as one launch (1: k_attention_b,
    256 threads, 8 blocks per chunk), inside the attention-LSTM launch (2, the default: 512 threads, 4 blocks) and that one without
    the tail form (XDTTS_NO_TAIL=1): one step and three steps, the same metric.
    Measured on an MI355X, the chunk closest to its bound per form, err(gpu, f64) | d32 | bound:
      XDTTS_ATT_FUSED=0  alignment 3.20e-07 | 1.72e-07 | 1.69e-06 (B = 17, T = 128)   rest 3.02e-07 | 1.10e-07 | 1.44e-06 (decoder_cell, B = 17, T = 100)
      XDTTS_ATT_FUSED=1  alignment 2.64e-07 | 9.40e-08 | 1.38e-06 (B = 17, T = 128)   rest 3.02e-07 | 1.10e-07 | 1.44e-06 (decoder_cell, B = 17, T = 100)
      XDTTS_ATT_FUSED=2  alignment 3.16e-07 | 1.79e-07 | 1.72e-06 (B = 17, T = 128)   rest 3.14e-07 | 1.32e-07 | 1.53e-06 (decoder_cell, B = 17, T = 257)
      XDTTS_NO_TAIL=1    alignment 2.89e-07 | 2.07e-07 | 1.83e-06 (B = 17, T = 512)   rest 3.14e-07 | 1.32e-07 | 1.53e-06 (decoder_cell, B = 17, T = 257)"""
    m = form_handles[form]
    for n in (1, 3):
        dw.check_case(m, _opts(pkg), orc, orc64, blob, "batched", B, T, dw.STEP0, n, _record, tag=form, **PLAN_KW[form])
    if form.startswith("fused"):
        assert m.engine_state()["batched_attention"] == int(form[-1]), m.engine_state()


PUBLIC = [(B, T) for T in (1, 16, 65, 128) for B in (1, 2, 5, 12)] + [(B, T) for T in (129, 256, 257, 512) for B in (1, 5, 17)]
_PUB = {}


def _public_ref(orc, orc64, blob, T, b):
    """ids, fixed steps, the fp64 mel of chunk b of window T and the fp32 oracle's worst frame against it."""
    if (T, b) not in _PUB:
        n = dw.n_valid_pool(T)[b]
        ids, steps = synth_ids(n, seed=1000 * T + b), 6 + (5 * b) % 7
        m64 = orc64.infer_chunk(blob, ids, orc64.default_opts(fixed_steps=steps, dropout_seed=dw.DROPOUT_SEED, item=b), window=T)
        m32 = orc.infer_chunk(blob, ids, orc.default_opts(fixed_steps=steps, dropout_seed=dw.DROPOUT_SEED, item=b), window=T)
        assert m64.shape == m32.shape == (80, steps)
        _PUB[(T, b)] = (ids, steps, m64, float(per_row_rel(m32, m64, 0).max()))
    return _PUB[(T, b)]


def _public_refs(orc, orc64, blob, T, B):
    """The references of a batch on a few threads (the oracle runs outside the interpreter lock): a chunk of a 512-id window is 2 s."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda b: _public_ref(orc, orc64, blob, T, b), range(B)))


@pytest.fixture(scope="module")
def public_handle(pkg, blob):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    m = pkg.Tacotron2.from_blob(blob)
    yield m
    m.close()


@pytest.mark.parametrize("B,T", PUBLIC)
def test_public_entries_follow_the_window(pkg, public_handle, orc, orc64, blob, B, T):
    """infer_batch with max_chunk = T against orc64.infer_chunk(window = T): chunk lengths T, 1, T - 1 and the class edges below,
    6 .. 12 fixed steps each; per mel frame || gpu - f64 || / || f64 ||, the worst frame <= 4 d32 + 1e-6 (gemm_shapes.bound).  What
    the hook bypasses runs here: launch_dimgroup_transpose, the length sort of the batched path, the context-fold table at
    T != 100.  T <= 128: the persistent kernel (B = 1), the pair (2), the 8- and 16-slot kernels (5, 12); above: the launch-per-stage
    engine (1) and the batched engine (5, 17).
    Measured on an MI355X, the worst frame err(gpu, f64) | d32 | bound: 5.23e-07 | 1.54e-07 | 1.62e-06 (B = 17, T = 129) on the batched engine,
    4.32e-07 | 1.39e-07 | 1.55e-06 (B = 12, T = 1) on the 16-slot kernel, 4.16e-07 | 1.42e-07 | 1.57e-06 (B = 2, T = 1) on the pair,
    3.47e-07 | 1.28e-07 | 1.51e-06 (B = 1, T = 65) on the persistent kernel, 2.88e-07 | 1.50e-07 | 1.60e-06 (B = 1, T = 512) launch per stage."""
    m = public_handle
    refs = _public_refs(orc, orc64, blob, T, B)
    mels = m.infer_batch([r[0] for r in refs], opts=pkg.default_opts(dropout_seed=dw.DROPOUT_SEED, max_chunk=T), fixed_steps=[r[1] for r in refs])
    st = m.engine_state()
    worst = None
    fails = []
    for b, (ids, steps, m64, d32) in enumerate(refs):
        assert mels[b].shape == m64.shape == (80, steps) and np.all(np.isfinite(mels[b])), (B, T, b, mels[b].shape)
        e = float(per_row_rel(mels[b], m64, 0).max())
        w = (e / frame_bound(d32), e, d32, len(ids))
        worst = w if worst is None or w > worst else worst
        if e > frame_bound(d32):
            fails.append((b, len(ids), e, d32))
    print("decoder-windows public B=%2d T=%3d  worst frame err(gpu,f64) %.2e d32 %.2e bound %.2e (%d ids)  engines %s" % (
        B, T, worst[1], worst[2], frame_bound(worst[2]), worst[3], st), flush=True)
    _record("public/B%d/T%d" % (B, T), {"err": worst[1], "d32": worst[2], "bound": frame_bound(worst[2]), "ids": worst[3]})
    assert not fails, (B, T, fails)
    if T <= dw.PERSIST_T_MAX:
        assert st["decoder_persistent" if B <= 2 else "decoder_persistent8"] == 1, (B, T, st)
    elif B >= 5:
        assert st["batched_attention"] == 2, (B, T, st)
