"""The NumPy restatement of the candidate specification (tests/shooting_reference.py) against things it does not share code
with: the oracle's Philox, the published Random123 known answer, the word-level form of the p = 0.5 rule, and the planner's
order on hand-made rows.  CPU only."""
import numpy as np

import shooting_reference as S


def test_philox_equals_the_oracle():
    from oracle import oracle as O

    rng = np.random.default_rng(7)
    n = 300
    seeds = [0, 1, 0xFFFFFFFF, 0x1_0000_0000, 0xDEADBEEF_00000000, 0xFFFFFFFF_FFFFFFFF]
    env = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    env[:4] = [0, 0xFFFFFFFF, 0x1_0000_0000, 0xFFFFFFFF_FFFFFFFF]
    epi = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    blk = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    epi[:3], blk[:3] = [0, 0xFFFFFFFF, 1], [0xFFFFFFFF, 0, 1]
    for j in range(n):
        seed = seeds[j % len(seeds)] if j < 60 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        got = S.philox4x32_10(seed, env[j], epi[j], blk[j])
        assert np.array_equal(got, O.philox(seed, int(env[j]), int(epi[j]), int(blk[j]))), (seed, env[j], epi[j], blk[j])


def test_philox_known_answer():
    """Random123 kat_vectors, philox4x32-10 with the zero counter and key"""
    assert S.philox4x32_10(0, 0, 0, 0).tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_word_stream_is_block_m_over_4_word_m_mod_4():
    g, k = np.array([0, 5, 1 << 40], np.uint64), np.arange(3)
    w = S.words(0x5EED, g, k, 11)
    assert w.shape == (11, 3, 3) and w.dtype == np.uint32
    for m in (0, 3, 4, 7, 10):
        for a, gi in enumerate(g.tolist()):
            for kk in range(3):
                assert w[m, a, kk] == S.philox4x32_10(0x5EED, gi, kk, m >> 2)[m & 3]


def test_fair_coin_is_the_top_bit_rule():
    g = np.arange(40, dtype=np.uint64) + np.uint64(1 << 33)
    a = S.discrete(99, g, 9, 13)
    assert np.array_equal(a, S.discrete_top_bit(99, g, 9, 13))
    assert np.array_equal(a, S.discrete(99, g, 9, 13, prob=np.full((13, 40), 0.5, np.float32)))
    assert 0.45 < a.mean() < 0.55
    # probabilities 0 and 1 are certain: u lies in [0, 1)
    assert not S.discrete(99, g, 9, 13, prob=np.zeros((13, 40), np.float32)).any()
    assert S.discrete(99, g, 9, 13, prob=np.ones((13, 40), np.float32)).all()


def test_uniform_draws_lie_in_the_range_and_use_consecutive_words():
    g = np.arange(6, dtype=np.uint64)
    for lo, hi, A in ((-3.0, 3.0, 1), (-1.0, 1.0, 3), (-1.0, 1.0, 6)):
        v = S.uniform(3, g, 50, 9, A, lo, hi)
        assert v.shape == (9, 6, 50, A) and v.dtype == np.float32
        assert (v >= lo).all() and (v <= hi).all() and v.min() < lo + 0.05 * (hi - lo) and v.max() > hi - 0.05 * (hi - lo)
        w = S.words(3, g, np.arange(50), 9 * A)
        assert np.array_equal(v[2, :, :, A - 1], (lo + (hi - lo) * S.u01(w[2 * A + A - 1]).astype(np.float64)).astype(np.float32))
    # the extreme fields: u = 0 gives lo exactly, u = 1 - 2^-24 stays inside
    assert np.float32(-3.0 + 6.0 * float(S.u01(np.uint32(0xFFFFFFFF)))) <= np.float32(3.0)
    assert S.u01(np.uint32(0xFF)) == 0 and S.u01(np.uint32(0xFFFFFFFF)) == np.float32(1 - 2.0 ** -24)


def test_gaussian_mode_pairs_and_clipping():
    g = np.arange(4, dtype=np.uint64)
    H, K, A = 5, 2000, 3
    mean = np.zeros((H, 4, A), np.float32)
    z = S.gaussian_exact(8, g, K, H, A, -100.0, 100.0, mean, 1.0)
    assert z.shape == (H, 4, K, A) and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    # components c = 2q and 2q + 1 share a radius: z_c^2 + z_{c+1}^2 = -2 ln u1
    flat = np.moveaxis(z, -1, 1).reshape(H * A, 4, K)
    w = S.words(8, g, np.arange(K), 16)
    rad2 = -2.0 * np.log((S.field(w[0::2]).astype(np.float64) + 1.0) * 2.0 ** -24)
    assert np.allclose(flat[0] ** 2 + flat[1] ** 2, rad2[0], rtol=1e-12, atol=1e-12)
    assert np.allclose(flat[12] ** 2 + flat[13] ** 2, rad2[6], rtol=1e-12, atol=1e-12)
    c = S.gaussian_exact(8, g, K, H, A, -1.0, 1.0, mean + 0.5, 2.0)
    assert c.min() == -1.0 and c.max() == 1.0


def test_best_of_order():
    nan, inf = np.nan, np.inf
    rows = np.array([
        [1.0, 3.0, 3.0, 2.0],      # tie: the first maximum
        [nan, 1.0, 5.0, 5.0],      # NaN first
        [4.0, nan, 4.0, 1.0],      # NaN in the middle, tie around it
        [nan, nan, nan, nan],      # all NaN: index 0
        [-inf, nan, -inf, nan],    # -inf beats NaN, first -inf
        [nan, -inf, 2.0, inf],     # +inf is the maximum
        [inf, inf, nan, 0.0],      # tie at +inf
        [nan, nan, -inf, nan],     # the only number, however small
        [0.0, -0.0, 0.0, -0.0],    # signed zeros compare equal
    ])
    assert S.best_of(rows).tolist() == [1, 2, 0, 0, 0, 3, 0, 2, 0]
    # where no NaN is involved it is argmax's first maximum
    r = np.random.default_rng(0).integers(0, 4, (200, 9)).astype(np.float64)
    assert np.array_equal(S.best_of(r), r.argmax(1))
    assert S.best_of(np.array([[7.0]])).tolist() == [0]
