"""tests/policy_noise_reference.py held to the text it restates and to shooting_reference (no GPU): the epsilon-greedy flags are the
candidate specification's discrete draws, the component-to-pair mapping for odd counts and past the first Philox block, the identity
PolicyNoise.draws relies on, zero scale, and the log-std head's clamp."""
import types

import numpy as np
import pytest

import policy_noise_reference as NR
import policy_reference as PR
import shooting_reference as SR

G = np.arange(4000, 4000 + 37, dtype=np.uint64)
SEEDS = (5, 2 ** 64 - 2)  # the second wraps: seed + t is taken mod 2^64


def _policy(obs_dim, hidden, n_out, seed=0, out="clip"):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    if hidden == 0:
        return types.SimpleNamespace(w1=None, b1=None, w2=f(n_out, obs_dim), b2=f(n_out), out=out)
    return types.SimpleNamespace(w1=f(hidden, obs_dim), b1=f(hidden), w2=f(n_out, hidden), b2=f(n_out), out=out)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("eps", [0.0, 0.25, 1.0])
def test_flags_are_the_discrete_draws_of_the_candidate_specification(seed, eps):
    for t in (0, 1, 7):
        explore, coin = NR.eps_greedy_flags(seed, t, G, eps)
        prob = np.stack([np.full(len(G), eps, np.float32), np.full(len(G), 0.5, np.float32)])
        want = SR.discrete(NR.key(seed, t), G, 1, 2, prob=prob)[:, :, 0]
        assert np.array_equal(explore, want[0] != 0) and np.array_equal(coin, want[1] != 0)
    assert NR.key(2 ** 64 - 2, 7) == 5


def test_epsilon_zero_is_greedy_and_epsilon_one_is_the_coin():
    pol = _policy(4, 0, 1)  # affine: both actions occur among the rows
    x = np.random.default_rng(1).standard_normal((len(G), 4)).astype(np.float32)
    greedy = PR.mlp_actions(pol, x, -1, 1, True)
    assert 0 < greedy.sum() < len(G)
    for t in range(3):
        f0, f1 = NR.eps_greedy_flags(9, t, G, 0.0), NR.eps_greedy_flags(9, t, G, 1.0)
        assert not f0[0].any() and f1[0].all()
        assert np.array_equal(NR.noisy_actions(pol, None, x, -1, 1, True, flags=f0), greedy)
        assert np.array_equal(NR.noisy_actions(pol, None, x, -1, 1, True, flags=f1), f1[1].astype(np.int64))
    coins = np.concatenate([NR.eps_greedy_flags(9, t, G, 1.0)[1] for t in range(40)])
    assert 0.4 < coins.mean() < 0.6


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_out", [1, 3, 6])
def test_component_to_pair_mapping(seed, n_out):
    """z_q of step t is component q of the candidate specification's step-0 draw under the key seed + t; an odd count leaves the
    last pair's sine half unused, and components 4 and 5 read words 4 and 5: the SECOND Philox block"""
    t = 3
    z = NR.normals_exact(seed, t, G, n_out)
    want = SR.gaussian_exact(NR.key(seed, t), G, 1, 1, n_out, -np.inf, np.inf, np.zeros((1, len(G), n_out), np.float32), 1.0)[0, :, 0, :]
    assert np.array_equal(z, want)
    assert [NR.pair_of(q) for q in range(6)] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    w = NR.noise_words(seed, t, G, 8)
    blocks = SR.philox4x32_10(NR.key(seed, t), G[None, :], 0, np.arange(2, dtype=np.uint64)[:, None])  # [2, N, 4]
    assert np.array_equal(w, np.moveaxis(blocks, -1, 1).reshape(8, len(G)))
    if n_out == 6:
        a, b = SR.field(blocks[1, :, 0]).astype(np.float64), SR.field(blocks[1, :, 1]).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log((a + 1.0) * 2.0 ** -24))
        assert np.array_equal(z[:, 4], rad * np.cos(2.0 * np.pi * b * 2.0 ** -24)) and np.array_equal(z[:, 5], rad * np.sin(2.0 * np.pi * b * 2.0 ** -24))
    # distinct steps and distinct envs draw distinct normals
    assert not np.array_equal(z, NR.normals_exact(seed, t + 1, G, n_out)) and len(np.unique(z[:, 0])) == len(G)


def test_eight_times_the_clipped_eighth_is_the_normal():
    """what PolicyNoise.draws relies on: |z| <= 5.77, so 0.125 z (exact: a power of two) stays inside a ctrlrange of +-1 or +-3 and
    8 * clip(0.125 z) == z"""
    z = np.concatenate([NR.normals_exact(s, t, G, 6).ravel() for s in SEEDS for t in range(50)]).astype(np.float32)
    assert np.abs(z).max() <= 5.77 and np.abs(z).max() > 3.0
    for lo, hi in ((-1.0, 1.0), (-3.0, 3.0)):
        eighth = np.clip(np.float32(0.125) * z, np.float32(lo), np.float32(hi))
        assert eighth.dtype == np.float32 and np.abs(eighth).max() < 1.0
        assert np.array_equal(np.float32(8.0) * eighth, z)
    # the largest radius the generator can produce: u1 = 2^-24
    assert np.sqrt(-2.0 * np.log(2.0 ** -24)) < 5.77


@pytest.mark.parametrize("hidden,n_out", [(0, 1), (5, 3), (7, 6)])
def test_zero_scale_leaves_y_unchanged(hidden, n_out):
    pol = _policy(11, hidden, n_out)
    x = np.random.default_rng(2).standard_normal((len(G), 11)).astype(np.float32)
    z = NR.normals_exact(1, 0, G, n_out).astype(np.float32)
    noise = types.SimpleNamespace(mode="gauss", seed=1, std=np.zeros(n_out, np.float32))
    yn, y, s = NR.noisy_logits(pol, noise, x, z)
    assert np.array_equal(yn, y) and not s.any()
    assert np.array_equal(NR.noisy_actions(pol, noise, x, -1, 1, False, z=z), PR.mlp_actions(pol, x, -1, 1, False))
    noise.std = np.full(n_out, 0.5, np.float32)
    yn = NR.noisy_logits(pol, noise, x, z)[0]
    assert np.array_equal(yn, y + 0.5 * z.astype(np.float64)) and not np.array_equal(yn, y)


@pytest.mark.parametrize("hidden", [0, 5])
def test_the_head_clamps_at_both_ends(hidden):
    pol = _policy(4, hidden, 2)
    x = np.random.default_rng(3).standard_normal((len(G), 4)).astype(np.float32)
    n_in = hidden if hidden else 4
    head = lambda b: types.SimpleNamespace(mode="head", seed=0, ws=np.zeros((2, n_in), np.float32), bs=np.asarray(b, np.float32),
                                           log_std_min=-20.0, log_std_max=2.0)
    s = NR.head_scale(pol, head([50.0, -50.0]), x)
    assert (s[:, 0] == np.float32(np.exp(2.0))).all() and (s[:, 1] == np.float32(np.exp(-20.0))).all()
    s = NR.head_scale(pol, head([2.0, -20.0]), x)  # the ends themselves
    assert (s[:, 0] == np.float32(np.exp(2.0))).all() and (s[:, 1] == np.float32(np.exp(-20.0))).all()
    inside = NR.head_scale(pol, head([0.5, -1.25]), x)
    assert (inside[:, 0] == np.float32(np.exp(0.5))).all() and (inside[:, 1] == np.float32(np.exp(-1.25))).all()
    # with weights the head follows the hidden activations y reads: it is mlp_logits with (ws, bs) for (w2, b2)
    h = head([0.1, -0.2])
    h.ws = np.random.default_rng(4).standard_normal((2, n_in)).astype(np.float32)
    lq = PR.mlp_logits(types.SimpleNamespace(w1=pol.w1, b1=pol.b1, w2=h.ws, b2=h.bs), x)
    assert np.array_equal(NR.head_scale(pol, h, x), np.exp(np.clip(lq, -20.0, 2.0)).astype(np.float32))
    assert len(np.unique(NR.head_scale(pol, h, x)[:, 0])) > 1
