"""tests/cem_reference.py held to its own edge cases (no GPU): the yardstick of tests/test_gpu_cem.py."""
import numpy as np

import cem_reference as C
from shooting_reference import best_of

NAN, INF = float("nan"), float("inf")


def _cands(H, N, K, seed=0, A=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (H, N, K) + ((A,) if A else ())).astype(np.float32)


def test_ties_are_broken_by_k():
    r = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 1.0]])
    assert C.elite_order(r).tolist() == [[1, 2, 4, 0, 5, 3]]
    c = _cands(3, 1, 6)
    # the threshold falls inside the group of 3.0s, then inside the group of 1.0s: the lower k is admitted
    for M, want in ((1, [1]), (2, [1, 2]), (3, [1, 2, 4]), (4, [0, 1, 2, 4]), (5, [0, 1, 2, 4, 5])):
        out = C.cem(c, r, M)
        assert np.nonzero(out.members[0])[0].tolist() == want
        assert out.elite_return[0] == (3.0 if M <= 3 else 1.0) and out.best_index[0] == 1 and out.best_return[0] == 3.0
        assert np.array_equal(out.mean, c[:, :, want].astype(np.float64).mean(2).astype(np.float32))


def test_signed_zeros_tie():
    r = np.array([[-0.0, 0.0, -1.0, 0.0, -0.0]])
    assert C.elite_order(r).tolist() == [[0, 1, 3, 4, 2]]
    out = C.cem(_cands(2, 1, 5), r, 3)
    assert np.nonzero(out.members[0])[0].tolist() == [0, 1, 3]
    assert out.elite_return[0] == 0.0 and not np.signbit(out.elite_return[0])  # candidate 3's own +0.0
    assert np.signbit(C.cem(_cands(2, 1, 5), r, 1).elite_return[0])  # candidate 0's own -0.0


def test_nan_is_admitted_only_after_everything_else():
    r = np.array([[NAN, 2.0, NAN, -INF, 1.0], [NAN] * 5])
    assert C.elite_order(r).tolist() == [[1, 4, 3, 0, 2], [0, 1, 2, 3, 4]]
    c = _cands(3, 2, 5, 1)
    out = C.cem(c, r, 3)
    assert np.nonzero(out.members[0])[0].tolist() == [1, 3, 4] and out.elite_return[0] == -INF
    assert np.nonzero(out.members[1])[0].tolist() == [0, 1, 2] and np.isnan(out.elite_return[1])  # all NaN: the first M by k
    assert out.best_index.tolist() == [1, 0] and np.isnan(out.best_return[1])
    out = C.cem(c, r, 4)
    assert np.nonzero(out.members[0])[0].tolist() == [0, 1, 3, 4] and np.isnan(out.elite_return[0])
    assert np.isfinite(out.mean).all() and np.isfinite(out.std).all()


def test_infinities_are_ordinary_values():
    r = np.array([[0.0, INF, -INF, INF, 5.0, -INF]])
    assert C.elite_order(r).tolist() == [[1, 3, 4, 0, 2, 5]]
    out = C.cem(_cands(2, 1, 6), r, 5)
    assert np.nonzero(out.members[0])[0].tolist() == [0, 1, 2, 3, 4] and out.elite_return[0] == -INF and out.best_return[0] == INF


def test_one_elite_is_the_shooting_winner_and_all_elites_are_the_plain_moments():
    rng = np.random.default_rng(3)
    H, N, K = 5, 7, 23
    r = rng.normal(0, 2, (N, K)).round(1)  # rounded: ties occur
    r[2, 5] = r[3, :] = NAN
    r[4, 0] = INF
    assert len(np.unique(r[0])) < K
    for A in (None, 3):
        c = _cands(H, N, K, 4, A)
        nom = _cands(H, N, 1, 5, A)[:, :, 0]
        one = C.cem(c, r, 1, nominal=nom)
        win = best_of(r)
        assert np.array_equal(one.best_index, win) and np.array_equal(one.members, np.arange(K)[None] == win[:, None])
        assert np.array_equal(one.elite_return, one.best_return, equal_nan=True)
        picked = np.stack([c[:, i, win[i]] for i in range(N)], axis=1)
        assert np.abs(one.mean - picked).max() <= np.spacing(np.float32(1)) and (one.std == 0).all()
        every = C.cem(c, r, K, nominal=nom)
        assert every.members.all()
        c64 = c.astype(np.float64)
        assert np.abs(every.mean - c64.mean(2)).max() <= np.spacing(np.float32(1))
        assert np.abs(every.std - c64.std(2)).max() <= np.spacing(np.float32(1))  # the population value (ddof = 0)
        assert every.mean.shape == (H, N) + ((A,) if A else ()) and every.mean.dtype == np.float32 and every.std.dtype == np.float32


def test_zero_variance_gives_zero_exactly():
    """M = 4 equal values: S1 = 4 d and S2 = 4 fl(d^2) are exact, so the difference is an exact 0 whatever the shift (with the shift
    on the common value itself, d = 0, it is for every M: the sigma_map = 0 case of the GPU test)"""
    H, N, K = 4, 3, 9
    c = np.repeat(_cands(H, N, 1, 6), K, axis=2)  # every candidate of an env draws the same sequence
    r = np.random.default_rng(7).normal(size=(N, K))
    for nom in (None, _cands(H, N, 1, 8)[:, :, 0], c[:, :, 0]):
        out = C.cem(c, r, 4, nominal=nom, lo=-1.0, hi=1.0)
        assert (out.std == 0).all() and (out.std64 == 0).all()
        assert np.abs(out.mean - c[:, :, 0]).max() <= np.spacing(np.float32(1))
    out = C.cem(c, r, 7, nominal=c[:, :, 0])
    assert (out.std == 0).all() and np.array_equal(out.mean, c[:, :, 0])
    # the discrete envs: probabilities, m0 = 0
    bits = (np.random.default_rng(9).random((H, N, K)) < 0.5).astype(np.uint8)
    out = C.cem(bits, r, 3)
    assert np.array_equal(out.mean, ((bits * out.members[None]).sum(2) / 3.0).astype(np.float32))


def test_the_shift_keeps_a_collapsed_sigma_meaningful():
    """values m + 1e-7 * z around m = 0.7: the unshifted E[x^2] - E[x]^2 loses everything, the shifted form keeps the digits"""
    rng = np.random.default_rng(10)
    H, N, K = 2, 1, 64
    nom = np.full((H, N), 0.7, np.float32)
    c = (nom.astype(np.float64)[:, :, None] + 1e-7 * rng.normal(size=(H, N, K)))  # float64 spread kept (not rounded to float32)
    c32 = c.astype(np.float32)
    out = C.cem(c32, np.zeros((N, K)), K, nominal=nom)
    want = c32.astype(np.float64).std(2)
    assert (want > 0).all() and np.abs(out.std64 - want).max() <= 1e-6 * want.max()
