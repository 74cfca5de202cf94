"""GPU tests of the vocoder's analysis direction: audio -> STFT magnitude -> log-mel under the handle's conventions
(xdtts_griffinlim_analyze / _analyze_batch) and the spectral convergence against a target magnitude
(xdtts_griffinlim_spectral_convergence), against the fp64 oracle and through properties that need no oracle."""
import ctypes as C

import numpy as np
import pytest

from conftest import rms

pytestmark = pytest.mark.gpu


def chirps(n):
    """BASELINE.md config-5 signal: five linear chirps 100 Hz - 7 kHz plus a little noise (as in test_gpu_griffinlim_more.py;
    a one-sample signal has t[-1] == 0, so its sweep time is taken as 1 s instead of dividing 0 by 0: y = [noise])."""
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(3)
    T = t[-1] if n > 1 else 1.0
    y = sum(0.15 * np.sin(2 * np.pi * (f0 + 0.5 * (f1 - f0) * t / T) * t) for f0, f1 in ((100, 900), (400, 2500), (1200, 4000), (3000, 5500), (5000, 7000)))
    return (y + 0.01 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def voc(pkg):
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    v = pkg.create_griffin_lim(iters=30, seed=3)  # create_griffin_lim(), src/tacotron2/mod.rs:441-458: power 1.7
    yield v
    v.close()


@pytest.fixture(scope="module")
def ref(orc, orc64):
    """n -> (signal, fp64 oracle magnitude, fp32 oracle magnitude as float32), each computed once."""
    cache = {}

    def get(n):
        if n not in cache:
            y = chirps(n)
            s64, s32 = orc64.stft(y), orc.stft(y)
            m32 = np.hypot(s32[..., 0], s32[..., 1])
            assert m32.dtype == np.float32
            cache[n] = (y, np.hypot(s64[..., 0], s64[..., 1]), m32)
            for a in cache[n]:
                a.setflags(write=False)
        return cache[n]

    return get


def mel_chain(B, m, power_mode, decompress, dtype, floor=1e-5):
    """The analysis chain behind the magnitude in `dtype`: exponent (the handle's, inverted), mel basis, compression."""
    e = {0: 1.7, 1: 1.0 / 1.7, 2: 1.0}[power_mode]
    p = m.astype(dtype) if e == 1.0 else m.astype(dtype) ** dtype(e)
    mel = B.astype(dtype) @ p
    assert mel.dtype == dtype
    if decompress == 1:
        return mel
    return (np.log if decompress == 0 else np.log10)(np.maximum(mel, dtype(floor)))


@pytest.mark.parametrize("n", [1, 2, 300, 1000, 2125, 9216])
def test_magnitude_matches_the_fp64_oracle(voc, ref, n):
    """F = 1, 1, 2, 4, 9, 37: reflect padding that folds many times (n <= 512; every index 0 at n = 1), n not a multiple of the
    hop, a partial last workgroup, more than one workgroup.  The GPU is no further from the fp64 oracle than twice the fp32
    oracle (+ 1e-6 of the signal's scale), and within 2e-5 of that scale.
    Measured on an MI355X, err(gpu, f64) / s | err(orc32, f64) / s (the test prints them):
      n = 1: 1.32e-07 | 1.35e-07    n = 2: 4.7e-08 | 6.2e-08    n = 300: 9.6e-08 | 1.02e-07
      n = 1000: 9.2e-08 | 9.6e-08    n = 2125: 9.5e-08 | 9.5e-08    n = 9216: 9.4e-08 | 9.9e-08
    so the first bound (2 x the fp32 oracle's own error + 1e-6 s, i.e. about 1.2e-6 s) is the binding one with a factor 12 to
    spare, mostly the issue's 1e-6 s term; the 2e-5 s bound is 200 x the measurement."""
    y, m64, m32 = ref(n)
    F = n // 256 + 1
    S, mel = voc.analyze(y, want_mel=False)
    assert mel is None and S.shape == (513, F) == m64.shape and S.dtype == np.float32 and np.all(np.isfinite(S))
    s = rms(m64, 0 * m64)
    eg, ef = rms(S, m64), rms(m32, m64)
    print("magnitude n=%d F=%d: err(gpu,f64)/s %.3e  err(orc32,f64)/s %.3e" % (n, F, eg / s, ef / s))
    assert eg <= 2.0 * ef + 1e-6 * s, (eg, ef, s)
    assert eg <= 2e-5 * s, (eg, s)


@pytest.mark.parametrize("n", [300, 1000, 2125, 9216])
def test_log_mel_matches_the_fp64_chain(voc, orc, ref, n):
    """ln(max(B @ S^1.7, 1e-5)) of the fp64 oracle magnitude, every cell; the yardstick d32 is the max abs distance of the
    same chain restated in float32 (fp32 oracle STFT, float32 hypot, ** 1.7, matmul, log) from fp64, and the GPU may be
    4 x d32 + 1e-6 away (its GEMM accumulates in another order than numpy's).
    Measured on an MI355X, max|gpu - f64| | d32 (the test prints them):
      n = 300: 5.5e-07 | 5.5e-07    n = 1000: 1.74e-06 | 1.84e-06    n = 2125: 4.50e-06 | 5.16e-06    n = 9216: 1.25e-05 | 9.5e-06
    -- the GPU is as far from fp64 as the float32 restatement is (0.9 .. 1.3 x d32), so the factor 4 has 3 x to spare; the
    error grows with n because the smallest cell falls (1.5e-2 at n = 300, 1.7e-4 at n = 9216) and ln magnifies it."""
    y, m64, m32 = ref(n)
    B = orc.mel_filter_bank()
    want = mel_chain(B, m64, 0, 0, np.float64)
    d32 = float(np.abs(mel_chain(B, m32, 0, 0, np.float32) - want).max())
    S, mel = voc.analyze(y, want_S=False)
    assert S is None and mel.shape == (80, n // 256 + 1) and np.all(np.isfinite(mel))
    dg = float(np.abs(mel - want).max())
    print("log-mel n=%d: max|gpu-f64| %.3e  d32 %.3e  (smallest cell %.3e)" % (n, dg, d32, float(np.exp(want.min()))))
    assert dg <= 4.0 * d32 + 1e-6, (dg, d32)


@pytest.mark.parametrize("kw", [dict(power_mode=1), dict(power_mode=2), dict(mel_decompress=1), dict(mel_decompress=2)],
                         ids=lambda kw: "%s%d" % next(iter(kw.items())))
def test_mel_under_the_other_conventions(pkg, orc, ref, kw):
    """Each other power_mode / mel_decompress setting once at n = 2125, under the rule of the test above (for mel_decompress = 1
    the cells are linear mel values, and so is the yardstick).
    Measured on an MI355X, max|gpu - f64| | d32 (the test prints them):
      power_mode 1: 1.87e-06 | 2.94e-06    power_mode 2: 3.02e-06 | 3.18e-06
      mel_decompress 1: 1.37e-06 | 1.37e-06    mel_decompress 2: 1.88e-06 | 2.27e-06"""
    y, m64, m32 = ref(2125)
    full = dict(power_mode=0, mel_decompress=0)
    full.update(kw)
    B = orc.mel_filter_bank()
    want = mel_chain(B, m64, full["power_mode"], full["mel_decompress"], np.float64)
    d32 = float(np.abs(mel_chain(B, m32, full["power_mode"], full["mel_decompress"], np.float32) - want).max())
    v = pkg.create_griffin_lim(iters=4, seed=1)
    try:
        v.set_opts(**full)
        _, mel = v.analyze(y, want_S=False)
    finally:
        v.close()
    dg = float(np.abs(mel - want).max())
    print("mel %s: max|gpu-f64| %.3e  d32 %.3e" % (kw, dg, d32))
    assert np.all(np.isfinite(mel)) and dg <= 4.0 * d32 + 1e-6, (kw, dg, d32)


def test_linear_mel_is_the_basis_times_the_gpus_own_magnitude(pkg, orc, ref):
    """power_mode 2, mel_decompress 1: mel_out = B @ S_out exactly as a statement about the projection alone (fp64 on the host
    from the GPU's own S): relative RMS <= 2e-5.  The mel floor plays no part in this mode."""
    y = ref(2125)[0]
    v = pkg.create_griffin_lim(iters=4, seed=1)
    try:
        v.set_opts(power_mode=2, mel_decompress=1)
        S, mel = v.analyze(y, mel_floor=0.5)
    finally:
        v.close()
    want = orc.mel_filter_bank().astype(np.float64) @ S.astype(np.float64)
    rel = rms(mel, want) / rms(want, 0 * want)
    print("projection alone: relative rms %.3e" % rel)
    assert rel <= 2e-5, rel


def test_batch_equals_the_single_calls_bit_for_bit(voc):
    lens = [9216, 300, 1, 2125, 1000, 5000]
    ys = [chirps(n) for n in lens]
    one = [voc.analyze(y) for y in ys]
    for order in (list(range(len(ys))), list(range(len(ys)))[::-1]):
        S, mel = voc.analyze_batch([ys[i] for i in order])
        for j, i in enumerate(order):
            assert S[j].shape == (513, lens[i] // 256 + 1) and mel[j].shape == (80, lens[i] // 256 + 1)
            assert np.array_equal(S[j], one[i][0]) and np.array_equal(mel[j], one[i][1]), (order, lens[i])
    # more than 80 rows in all: the mel GEMM maps blocks to tiles by XCD from there on; the bits must not notice
    S, mel = voc.analyze_batch([ys[0], ys[3], ys[0], ys[5]])
    for j, i in enumerate((0, 3, 0, 5)):
        assert np.array_equal(S[j], one[i][0]) and np.array_equal(mel[j], one[i][1]), (j, lens[i])
    # only one of the two outputs, and the timings of the call
    S, mel = voc.analyze_batch(ys[:2], want_S=False)
    assert S is None and np.array_equal(mel[1], one[1][1])
    t = voc.analysis_timings()
    assert t["magnitude_ms"] > 0 and t["projection_ms"] > 0 and t["total_ms"] >= t["magnitude_ms"]


def test_spectral_convergence_matches_fp64_and_is_deterministic(voc, orc64, ref):
    """Target S = the fp64 oracle magnitude of the chirps at F = 37 (as float32, what the entry takes).
    - a perturbed signal y2 = y + 0.05 noise: the device value equals || |STFT64(y2)| - S || / || S || within 1e-5 relative
      (the magnitudes feeding the sums are good to 1e-7 of the scale, so this isolates the fixed-order fp64 reduction;
      measured: device 1.756739914e-01, fp64 1.756739960e-01, 2.6e-08 relative);
    - y itself: below 1e-5 (S is its own magnitude up to rounding; measured 9.6e-08 on an MI355X, a hundredth of the bound);
    - the least-squares gain.  For S = y's own magnitude, 0.3 y gives a = 1 / 0.3 within 1e-5 and the distance of y.  For y2 the
      fitted gain is <|X2|, S> / <|X2|, |X2|>, which is not 1 (y2 is not S's signal), so what scaling by 0.3 must do there is
      divide that gain by 0.3 and leave the distance alone: both to 1e-5 relative, and both equal to their fp64 restatement;
    - two calls return the same bits."""
    y, m64, _ = ref(9216)
    S = m64.astype(np.float32)
    S64 = S.astype(np.float64)
    y2 = (y + 0.05 * np.random.default_rng(7).standard_normal(y.size)).astype(np.float32)
    r = orc64.stft(y2)
    X2 = np.hypot(r[..., 0], r[..., 1])
    nS = np.linalg.norm(S64)
    want = float(np.linalg.norm(X2 - S64) / nS)
    got, a = voc.spectral_convergence(y2, S)
    print("convergence y2: device %.9e  fp64 %.9e  rel %.2e" % (got, want, abs(got - want) / want))
    assert a == 1.0 and abs(got - want) <= 1e-5 * want, (got, want)
    own, a = voc.spectral_convergence(y, S)
    print("convergence y against its own magnitude: %.3e" % own)
    assert a == 1.0 and 0.0 <= own < 1e-5, own
    # gain: literally 1 / 0.3 where S is the signal's own magnitude
    d03, a03 = voc.spectral_convergence(np.float32(0.3) * y, S, fit_gain=True)
    print("gain of 0.3 y: %.8f (1 / 0.3 = %.8f), distance %.3e" % (a03, 1 / 0.3, d03))
    assert abs(a03 - 1.0 / 0.3) <= 1e-5 and d03 < 1e-5
    # ... and for y2: the fp64 least-squares gain, scaled by 1 / 0.3, the distance unchanged
    a_want = float(np.sum(X2 * S64) / np.sum(X2 * X2))
    d_want = float(np.linalg.norm(a_want * X2 - S64) / nS)
    d2, a2 = voc.spectral_convergence(y2, S, fit_gain=True)
    d2s, a2s = voc.spectral_convergence(np.float32(0.3) * y2, S, fit_gain=True)
    print("gain y2: device %.8f fp64 %.8f; distance device %.9e fp64 %.9e; 0.3 y2: gain %.8f distance %.9e" % (a2, a_want, d2, d_want, a2s, d2s))
    assert abs(a2 - a_want) <= 1e-5 * a_want and abs(d2 - d_want) <= 1e-5 * d_want
    assert abs(a2s - a2 / 0.3) <= 1e-5 * a2 / 0.3 and abs(d2s - d2) <= 1e-5 * d2
    assert d2 <= got  # the fitted gain cannot do worse than a = 1
    # determinism
    assert voc.spectral_convergence(y2, S) == (got, 1.0) and voc.spectral_convergence(y2, S, fit_gain=True) == (d2, a2)
    t = voc.analysis_timings()
    assert t["magnitude_ms"] > 0 and t["projection_ms"] > 0


def test_convergence_falls_with_the_iteration_count(voc, ref):
    """The property of test_config5_full_size_properties at F = 37, with no oracle in the loop."""
    S = ref(9216)[1].astype(np.float32)
    voc.set_seed(3)
    c = [voc.spectral_convergence(voc.infer_linear(S, iters=k), S)[0] for k in (2, 10, 30)]
    print("convergence after 2 / 10 / 30 iterations: %.4f %.4f %.4f" % tuple(c))
    assert c[0] > c[1] > c[2] > 0.0, c


def test_round_trip_through_the_product_only(pkg):
    """mel -> audio -> mel with no oracle: the 40-frame mel of test_full_infer_from_mel, output_normalise off."""
    rng = np.random.default_rng(11)
    F = 40
    mel = (rng.uniform(-7.0, -1.0, size=(80, F)) + 2.0 * np.sin(np.arange(F) / 5.0)[None, :]).astype(np.float32)
    v = pkg.create_griffin_lim(iters=30, seed=5)
    try:
        v.set_opts(output_normalise=0)
        audio = v.infer(mel)
        S_a, mel_a = v.analyze(audio)
        assert S_a.shape == (513, F) and mel_a.shape == (80, F) and np.all(np.isfinite(mel_a)) and np.all(np.isfinite(S_a))
        S = v.mel_to_linear(mel)
        c30 = v.spectral_convergence(audio, S)[0]
        c2 = v.spectral_convergence(v.infer_linear(S, iters=2), S)[0]
    finally:
        v.close()
    print("round trip: convergence after 30 iterations %.4f, after 2 %.4f" % (c30, c2))
    assert 0.0 < c30 < c2, (c30, c2)


def test_errors(pkg, voc, ref):
    y, m64, _ = ref(9216)
    S = m64.astype(np.float32)
    for bad_S in (S[:, :36], np.concatenate([S, S[:, :1]], axis=1), np.zeros_like(S)):  # wrong frame counts, an all-zero target
        with pytest.raises(pkg.XdttsError) as e:
            voc.spectral_convergence(y, bad_S)
        assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    with pytest.raises(pkg.XdttsError) as e:
        voc.analyze(np.zeros(0, dtype=np.float32))
    assert e.value.status == pkg.XDTTS_ERR_BAD_ARG
    # a live handle with no samples / no utterances / null pointers
    lib, h = pkg.lib, voc._h
    p = y.ctypes.data_as(C.c_void_p)
    out = (C.c_float * 2)()
    assert lib.xdtts_griffinlim_spectral_convergence(h, p, 0, S.ctypes.data_as(C.c_void_p), 1, 0, C.byref(out)) == pkg.XDTTS_ERR_BAD_ARG
    assert lib.xdtts_griffinlim_spectral_convergence(h, p, y.size, None, 37, 0, C.byref(out)) == pkg.XDTTS_ERR_BAD_ARG
    assert lib.xdtts_griffinlim_spectral_convergence(h, p, y.size, S.ctypes.data_as(C.c_void_p), 37, 2, C.byref(out)) == pkg.XDTTS_ERR_BAD_ARG
    ptrs, ns = (C.c_void_p * 1)(y.ctypes.data), (C.c_size_t * 1)(y.size)
    assert lib.xdtts_griffinlim_analyze_batch(h, ptrs, ns, 0, 1e-5, None, None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert lib.xdtts_griffinlim_analyze_batch(h, None, ns, 1, 1e-5, None, None, None) == pkg.XDTTS_ERR_BAD_ARG
    assert lib.xdtts_griffinlim_analyze(h, None, y.size, 1e-5, None, None, None) == pkg.XDTTS_ERR_BAD_ARG
    # and the handle still works
    assert voc.spectral_convergence(y, S)[0] < 1e-5
