"""The SPSI initial phase (phase_init mode 1) as tests/spsi_ref.py restates it: the segment scan against the sequential
recurrence, the frames and bins the definition singles out, and the property the stage exists for -- a lower spectral
convergence than a random start at a small iteration budget, here in fp64.  No GPU."""
import numpy as np
import pytest

import prosody_ref as pr
import spsi_ref as sr


@pytest.fixture(scope="module")
def voiced():
    """|STFT| of the voiced test signal, (513, 48) fp64; read-only."""
    S = pr.stft_magnitude(pr.voiced_signal(256 * 47))
    S.setflags(write=False)
    return S


@pytest.mark.parametrize("F", [1, 2, 3, 17, 48])
def test_scanned_equals_sequential(voiced, F):
    """Any segmentation gives the bits of the frame-by-frame recurrence: random magnitudes (5 % exact zeros, so flat pairs
    and ties between two peaks occur) and the voiced magnitude."""
    for name, S in (("random", pr.random_magnitude(F, seed=40 + F)), ("voiced", voiced[:, :F].astype(np.float32))):
        own, delta = sr.frame_maps(S)
        assert own.shape == delta.shape == (F, 513) and delta.dtype == np.uint32
        assert own.min() >= 0 and own.max() <= 512
        seq = sr.sequential(own, delta)
        assert seq.dtype == np.uint32
        for L in (1, 2, 7, 16):
            assert np.array_equal(sr.scanned(own, delta, L), seq), (name, F, L)


def test_ties_go_to_the_lower_peak():
    m = np.zeros((513, 1), dtype=np.float32)
    m[10, 0] = m[14, 0] = 1.0
    own, _ = sr.frame_maps(m)
    assert own[0, 12] == 10 and own[0, 11] == 10 and own[0, 13] == 14 and own[0, 10] == 10 and own[0, 14] == 14
    assert own[0, 0] == 10 and own[0, 512] == 14
    # a flat pair: the lower bin is the peak (m[k] > m[k-1] and m[k] >= m[k+1]), the upper one is not
    m[:, 0] = 0.0
    m[20, 0] = m[21, 0] = 1.0
    own, delta = sr.frame_maps(m)
    # a = 0, c = b = 1: d = -1, p = 0.5 * (0 - 1) / -1 = 0.5 (the clamp's edge); 20 & 3 == 0, so adv = 0.5 * 2^30
    assert (own[0] == 20).all() and delta[0, 20] == 1 << 29


def test_a_frame_of_zeros_carries_the_phase_through():
    S = pr.random_magnitude(5, seed=3)
    S[:, 2] = 0.0
    t = sr.turns(S)
    assert np.array_equal(t[:, 2], t[:, 1]) and not np.array_equal(t[:, 1], t[:, 0]) and not np.array_equal(t[:, 3], t[:, 2])


def test_an_all_zero_utterance_gives_turns_zero():
    t = sr.turns(np.zeros((513, 4), dtype=np.float32))
    assert t.dtype == np.uint32 and not t.any()
    a = sr.angles(t)
    assert np.array_equal(a[..., 0], np.ones((513, 4))) and not a[..., 1].any()


def test_bins_0_and_512_are_never_peaks():
    S = pr.random_magnitude(6, seed=9)
    S[0, :] = 10.0
    S[512, :] = 10.0
    own, _ = sr.frame_maps(S)
    assert not (own == 0).any() and not (own == 512).any()
    # ... and they follow their nearest peak like any other bin
    assert (own[:, 0] >= 1).all() and (own[:, 512] <= 511).all()


def test_the_half_turn_of_the_main_lobe():
    """One stationary sinusoid between bins 40 and 41, nearer 40 (p > 0): the bins below the peak and the one just above it
    are half a turn away from the peak, the bins further above are in phase with it."""
    m = np.zeros((513, 1), dtype=np.float32)
    m[39:43, 0] = (0.3, 1.0, 0.6, 0.1)
    own, delta = sr.frame_maps(m)
    assert (own[0] == 40).all()
    d = delta[0].astype(np.int64)
    assert d[40] < (1 << 29) and d[40] > 0  # 40 & 3 == 0: the advance is p / 4 turns... p * 2^30 units, 0 < p <= 0.5
    half = (d - d[40]) % (1 << 32)
    assert (half[:40] == 1 << 31).all() and half[41] == 1 << 31 and (half[42:] == 0).all()


def test_spsi_beats_a_random_start_at_a_small_budget(voiced):
    """SC_spsi(K) <= 0.6 SC_rand(K) at K = 2 and <= 0.8 SC_rand(K) at K = 5, for three random seeds, fp64 fast Griffin-Lim
    under the handle's conventions on the voiced magnitude (F = 48).  Measured: ratios 0.43 .. 0.50 and 0.45 .. 0.53
    (SPSI 0.153 / 0.124; random 0.31 .. 0.36 / 0.23 .. 0.28); without any iteration 0.204 against 0.64 .. 0.65."""
    a1 = sr.spsi_angles(voiced)
    for K, factor in ((2, 0.6), (5, 0.8)):
        sc1 = sr.spectral_convergence(sr.griffinlim(voiced, a1, K), voiced)
        for seed in (0, 1, 2):
            sc0 = sr.spectral_convergence(sr.griffinlim(voiced, sr.random_angles(48, seed), K), voiced)
            print("K=%d seed=%d: random %.4f  spsi %.4f  ratio %.3f" % (K, seed, sc0, sc1, sc1 / sc0))
            assert sc1 <= factor * sc0, (K, seed, sc1, sc0)
