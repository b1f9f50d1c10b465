"""tests/mppi_reference.py held to its own edge cases (no GPU): the yardstick of tests/test_gpu_mppi.py."""
import math

import numpy as np

import mppi_reference as M

NAN, INF = float("nan"), float("inf")


def _cands(H, N, K, seed=0, A=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (H, N, K) + ((A,) if A else ())).astype(np.float32)


def test_finite_returns_equal_a_plain_softmax():
    rng = np.random.default_rng(1)
    H, N, K = 6, 5, 17
    for A in (None, 3):
        c = _cands(H, N, K, 2, A)
        r = rng.normal(0, 3, (N, K))
        for T in (0.1, 1.0, 7.5):
            out, br, bi, ess = M.mppi(c, r, T)
            e = np.exp((r - r.max(1, keepdims=True)) / T)
            p = e / e.sum(1, keepdims=True)
            want = np.einsum("nk,hnk...->hn...", p, c.astype(np.float64))
            assert out.dtype == np.float32 and out.shape == (H, N) + ((A,) if A else ())
            assert np.abs(out - want).max() <= np.spacing(np.float32(1))
            assert np.array_equal(bi, r.argmax(1)) and np.array_equal(br, r.max(1))
            assert np.allclose(ess, 1.0 / (p * p).sum(1), rtol=1e-12, atol=0)
            assert (ess >= 1.0 - 1e-12).all() and (ess <= K + 1e-9).all()


def test_ties_share_the_weight():
    r = np.array([[1.0, 3.0, 3.0, -2.0, 3.0]])
    w, best = M.weights(r, 0.5)
    assert best[0] == 1 and np.array_equal(w[0, [1, 2, 4]], [1.0, 1.0, 1.0])
    assert w[0, 0] == math.exp(-4.0) and w[0, 3] == math.exp(-10.0)
    c = _cands(3, 1, 5)
    out, br, bi, ess = M.mppi(c, r, 1e-300)
    assert np.array_equal(out, c[:, :, [1, 2, 4]].astype(np.float64).mean(2).astype(np.float32))
    assert ess[0] == 3.0 and br[0] == 3.0 and bi[0] == 1


def test_infinite_returns():
    # a +inf maximum: the +inf candidates share the weight, everything finite gets exp(-inf) = 0; -inf entries weigh 0
    r = np.array([[0.0, INF, -INF, INF, 5.0], [-INF, 2.0, 1.0, -INF, 2.0], [-INF] * 5])
    w, best = M.weights(r, 1.0)
    assert np.array_equal(w[0], [0.0, 1.0, 0.0, 1.0, 0.0]) and best[0] == 1
    assert np.array_equal(w[1], [0.0, 1.0, math.exp(-1.0), 0.0, 1.0]) and best[1] == 1
    assert np.array_equal(w[2], [1.0] * 5) and best[2] == 0  # a row of all -inf: every candidate is a maximiser
    c = _cands(4, 3, 5, 3)
    out, br, bi, ess = M.mppi(c, r, 1.0)
    assert np.array_equal(out[:, 0], c[:, 0, [1, 3]].astype(np.float64).mean(1).astype(np.float32))
    assert np.array_equal(out[:, 2], c[:, 2].astype(np.float64).mean(1).astype(np.float32))
    assert ess[0] == 2.0 and ess[2] == 5.0 and br[0] == INF and br[2] == -INF
    assert np.isfinite(out).all()


def test_nan_returns():
    r = np.array([[NAN, 1.0, NAN, 0.0], [NAN] * 4, [NAN, -INF, NAN, NAN]])
    w, best = M.weights(r, 2.0)
    assert np.array_equal(w[0], [0.0, 1.0, 0.0, math.exp(-0.5)]) and best[0] == 1
    assert np.array_equal(w[1], [1.0] * 4) and best[1] == 0  # all NaN: the uniform mean
    assert np.array_equal(w[2], [0.0, 1.0, 0.0, 0.0]) and best[2] == 1  # -inf beats NaN
    c = _cands(2, 3, 4, 4)
    out, br, bi, ess = M.mppi(c, r, 2.0)
    assert np.array_equal(out[:, 1], c[:, 1].astype(np.float64).mean(1).astype(np.float32))
    assert np.array_equal(out[:, 2], c[:, 2, 1])
    assert np.isnan(br[1]) and bi[1] == 0 and ess[1] == 4.0 and ess[2] == 1.0
    assert np.isfinite(out).all() and np.isfinite(ess).all()


def test_single_candidate():
    for r0 in (0.3, NAN, INF, -INF):
        c = _cands(5, 2, 1, 5)
        out, br, bi, ess = M.mppi(c, np.full((2, 1), r0), 0.7)
        assert np.array_equal(out, c[:, :, 0]) and (bi == 0).all() and (ess == 1.0).all()
        assert np.array_equal(br, [r0, r0], equal_nan=True)


def test_temperature_limits():
    rng = np.random.default_rng(6)
    N, K = 6, 11
    r = rng.integers(0, 4, (N, K)).astype(np.float64)  # integers: shared maxima
    r[0, 3] = r[2, 0] = r[2, 7] = NAN
    r[4] = NAN
    c = _cands(3, N, K, 7, A=2).astype(np.float64)
    cold, _, _, ess_cold = M.mppi(c, r, 1e-300)
    hot, _, _, ess_hot = M.mppi(c, r, 1e300)
    for i in range(N):
        ok = ~np.isnan(r[i])
        maxi = ok & (r[i] == np.nanmax(r[i])) if ok.any() else np.ones(K, bool)
        live = ok if ok.any() else np.ones(K, bool)
        assert np.array_equal(cold[:, i], c[:, i, maxi].mean(1).astype(np.float32))
        assert ess_cold[i] == maxi.sum()
        assert np.abs(hot[:, i] - c[:, i, live].mean(1)).max() <= np.spacing(np.float32(1))
        assert abs(ess_hot[i] - live.sum()) <= 1e-12 * K
    assert (np.sum(~np.isnan(r), 1)[[0, 2]] == [K - 1, K - 2]).all()
