"""tests/policy_reference.py:mlp_actions, the numpy form of emei_rollout_policy's normative policy arithmetic, checked on the CPU:
against torch float64 modules on random weights, on the NaN / +-inf / exact-zero cases the text spells out, and for its sensitivity
to the summation order (so that the bit-for-bit GPU tests can tell a kernel that sums in another order).

The normative hidden unit is ROUNDED TO FLOAT32 before the ReLU (h_j = (float)z).  A plain float64 Sequential(Linear, ReLU, Linear)
keeps it in float64, so its outputs differ from the text's by up to sum_j |w2[q,j]| * |h_j| * 2^-24 — most of a float32 spacing of
y for 64 hidden units: "equal after rounding to float32" cannot hold against it.  The exact comparison therefore runs against the
float64 Sequential with that one rounding made explicit (a module between Linear and ReLU); the plain Sequential is held to the
derived bound."""
import numpy as np
import pytest

import policy_reference as P

torch = pytest.importorskip("torch")


class _Pol:
    def __init__(self, w2, b2, w1=None, b1=None, out="clip"):
        self.w1, self.b1, self.w2, self.b2, self.out = w1, b1, w2, b2, out


class _RoundF32(torch.nn.Module):
    def forward(self, z):
        return z.to(torch.float32).to(torch.float64)


def _random_policy(rng, obs_dim, hidden, n_out, scale=1.0):
    f = lambda *s: (rng.standard_normal(s) * scale / np.sqrt(s[-1])).astype(np.float32)
    if hidden == 0:
        return _Pol(f(n_out, obs_dim), f(n_out).reshape(n_out))
    return _Pol(f(n_out, hidden), f(n_out).reshape(n_out), f(hidden, obs_dim), f(hidden).reshape(hidden))


def _sequential(pol, rounded):
    lin = lambda w, b: torch.nn.Linear(w.shape[1], w.shape[0]).double()
    mods = []
    if pol.w1 is not None:
        l1 = lin(pol.w1, pol.b1)
        mods += [l1] + ([_RoundF32()] if rounded else []) + [torch.nn.ReLU()]
        with torch.no_grad():
            l1.weight.copy_(torch.as_tensor(pol.w1).double()), l1.bias.copy_(torch.as_tensor(pol.b1).double())
    l2 = lin(pol.w2, pol.b2)
    with torch.no_grad():
        l2.weight.copy_(torch.as_tensor(pol.w2).double()), l2.bias.copy_(torch.as_tensor(pol.b2).double())
    return torch.nn.Sequential(*(mods + [l2]))


@pytest.mark.parametrize("obs_dim,hidden,n_out", [(4, 0, 1), (4, 1, 1), (4, 5, 1), (4, 64, 1), (6, 64, 1), (17, 64, 6), (11, 5, 3), (17, 0, 6)])
def test_mlp_actions_against_torch_float64(obs_dim, hidden, n_out):
    rng = np.random.default_rng(100 * obs_dim + hidden)
    pol = _random_policy(rng, obs_dim, hidden, n_out, scale=2.0)
    x = rng.standard_normal((257, obs_dim)).astype(np.float32)
    lo, hi = np.float32(-1.0), np.float32(1.0)
    got = P.mlp_actions(pol, x, lo, hi, False)
    assert got.dtype == np.float32 and got.shape == (257, n_out)
    with torch.no_grad():
        y = _sequential(pol, rounded=True)(torch.as_tensor(x).double())
        want = torch.clamp(y.to(torch.float32), float(lo), float(hi)).numpy()
        y_plain = _sequential(pol, rounded=False)(torch.as_tensor(x).double()).numpy()
    assert np.array_equal(got, want)
    assert (np.abs(got) < 1.0).mean() > 0.1 and (np.abs(got) == 1.0).any()  # both sides of the clip are exercised
    # discrete: the sign of the first logit
    assert np.array_equal(P.mlp_actions(pol, x, lo, hi, True), (y[:, 0].numpy() >= 0).astype(np.int64))
    # the plain float64 Sequential: within the bound the one float32 rounding of h allows (module docstring)
    yy = P.mlp_logits(pol, x)
    if hidden:
        with torch.no_grad():
            h = torch.relu(_sequential(pol, True)[0](torch.as_tensor(x).double())).numpy()
        bound = (np.abs(h) @ np.abs(pol.w2.astype(np.float64)).T) * 2.0 ** -24
    else:
        bound = np.zeros_like(yy)
    assert (np.abs(yy - y_plain) <= bound + 1e-13 * (1.0 + np.abs(yy))).all()
    assert np.allclose(yy, y.numpy(), rtol=1e-13, atol=1e-13)


def test_special_values():
    lo, hi = np.float32(-3.0), np.float32(3.0)
    nan, inf = np.float32("nan"), np.float32("inf")
    # a NaN input: every hidden unit is NaN -> 0 after the ReLU, so the output is b2 alone
    pol = _Pol(np.float32([[1.0, -2.0]]), np.float32([0.25]), np.float32([[1, 1, 1, 1], [2, 0, 0, 0]]), np.float32([0.0, 1.0]))
    x = np.float32([[nan, 0, 0, 0], [1, 1, 1, 1]])
    assert np.array_equal(P.mlp_actions(pol, x, lo, hi, False), np.float32([[0.25], [4.0 - 6.0 + 0.25]]))
    assert np.array_equal(P.mlp_actions(pol, x, lo, hi, True), [1, 0])
    # an affine policy on NaN: y is NaN -> lo (continuous), 0 (discrete)
    aff = _Pol(np.float32([[1, 0, 0, 0]]), np.float32([0.0]))
    assert np.array_equal(P.mlp_actions(aff, x[:1], lo, hi, False), [[lo]]) and np.array_equal(P.mlp_actions(aff, x[:1], lo, hi, True), [0])
    # +-inf logits clip to the range; an infinite weight on a zero hidden unit is inf * 0 = NaN -> lo
    xi = np.float32([[inf, 0, 0, 0], [-inf, 0, 0, 0], [3e38, 0, 0, 0]])
    big = _Pol(np.float32([[3e38, 0, 0, 0]]), np.float32([0.0]))
    assert np.array_equal(P.mlp_actions(big, xi, lo, hi, False), [[hi], [lo], [hi]])  # 9e76 is finite in float64, +inf as float32
    assert np.array_equal(P.mlp_actions(big, xi, lo, hi, True), [1, 0, 1])
    infw = _Pol(np.float32([[inf, 1.0]]), np.float32([0.0]), np.float32([[-1, 0, 0, 0], [1, 0, 0, 0]]), np.float32([0.0, 0.0]))
    assert np.array_equal(P.mlp_actions(infw, np.float32([[2, 0, 0, 0]]), lo, hi, False), [[lo]])
    # an exactly zero logit is "up" (y >= 0), and so is -0.0
    zero = _Pol(np.float32([[1, -1, 0, 0]]), np.float32([0.0]))
    assert np.array_equal(P.mlp_actions(zero, np.float32([[0.5, 0.5, 9, 9], [0.5, 0.75, 0, 0]]), lo, hi, True), [1, 0])
    mz = _Pol(np.float32([[-1, 0, 0, 0]]), np.float32([-0.0]))
    assert np.array_equal(P.mlp_actions(mz, np.float32([[0, 0, 0, 0]]), lo, hi, True), [1])
    # a negative hidden unit is cut to 0, a positive one kept (rounded to float32 first)
    relu = _Pol(np.float32([[1.0]]), np.float32([0.0]), np.float32([[1, 0, 0, 0]]), np.float32([0.0]))
    assert np.array_equal(P.mlp_actions(relu, np.float32([[-2, 0, 0, 0], [0.5, 0, 0, 0]]), lo, hi, False), [[0.0], [0.5]])
    third = _Pol(np.float32([[1.0]]), np.float32([0.0]), np.float32([[np.float32(1 / 3), 0, 0, 0]]), np.float32([0.0]))
    got = P.mlp_logits(third, np.float32([[np.float32(1 / 3), 0, 0, 0]]))[0, 0]
    assert got == np.float64(np.float32(np.float64(np.float32(1 / 3)) ** 2))  # h rounded to float32 before it is used
    # tanh mode maps onto [lo, hi]
    th = _Pol(np.float32([[1, 0, 0, 0]]), np.float32([0.0]), out="tanh")
    a = P.mlp_actions(th, np.float32([[0, 0, 0, 0], [40, 0, 0, 0], [-40, 0, 0, 0], [0.5, 0, 0, 0]]), lo, hi, False)[:, 0]
    assert a[0] == 0 and a[1] == hi and a[2] == lo and a[3] == np.float32(3.0 * np.tanh(0.5))


def test_the_summation_order_shows():
    """ascending order is part of the specification: another order changes bits of the logits, and can change an action"""
    rng = np.random.default_rng(7)
    pol = _random_policy(rng, 6, 64, 1, scale=2.0)
    x = rng.standard_normal((512, 6)).astype(np.float32)
    asc = P.mlp_logits(pol, x)
    rev = P.mlp_logits(pol, x, order=list(range(63, -1, -1)))
    perm = P.mlp_logits(pol, x, order=list(rng.permutation(64)))
    for other in (rev, perm):
        changed = asc.view(np.uint64) != other.view(np.uint64)
        assert 0.05 < changed.mean() and np.allclose(asc, other, rtol=1e-12, atol=1e-13)
    # ... and an action: 2^60 - 1 - 2^60 is 0 in ascending order (the 1 is absorbed), -1 with the two large terms first
    big = np.float32(2.0 ** 60)
    aff = _Pol(np.float32([[big, -1.0, -big, 0.0]]), np.float32([0.0]))
    one = np.float32([[1, 1, 1, 1]])
    assert P.mlp_actions(aff, one, -1, 1, True)[0] == 1 and P.mlp_actions(aff, one, -1, 1, True, order=[0, 2, 1, 3])[0] == 0
    assert P.mlp_actions(aff, one, -1, 1, False)[0, 0] == 0.0 and P.mlp_actions(aff, one, -1, 1, False, order=[0, 2, 1, 3])[0, 0] == -1.0


def test_mlppolicy_call_is_the_reference():
    """MLPPolicy.__call__ (torch float64, what the per-step path of datasets.collect runs) gives mlp_actions' bits on the CPU"""
    from emei_amd.policy import MLPPolicy

    rng = np.random.default_rng(11)
    for obs_dim, hidden, n_out, discrete, name in ((4, 64, 1, True, "CartPoleSwingUp"), (4, 5, 1, False, "ReboundInvertedPendulumSwingUp"),
                                                   (17, 64, 6, False, "HalfCheetahRunning"), (6, 0, 1, False, "ReboundInvertedDoublePendulumSwingUp")):
        ref = _random_policy(rng, obs_dim, hidden, n_out, scale=3.0)
        pol = MLPPolicy(ref.w2, ref.b2, ref.w1, ref.b1)
        pol.discrete = discrete
        pol.lo, pol.hi = (float(v) for v in P.ctrl_range(name))
        x = rng.standard_normal((130, obs_dim)).astype(np.float32)
        x[3, 0] = np.nan
        got = pol(torch.as_tensor(x)).numpy()
        want = P.mlp_actions(ref, x, pol.lo, pol.hi, discrete)
        assert np.array_equal(got, want if (discrete or n_out > 1) else want[:, 0], equal_nan=True)
    seq = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1), torch.nn.Tanh())
    pol = MLPPolicy.from_module(seq)
    assert pol.out == "tanh" and pol.hidden == 8 and pol.obs_dim == 4 and pol.n_out == 1
    assert MLPPolicy.from_module(torch.nn.Sequential(torch.nn.Linear(17, 6))).hidden == 0
    with pytest.raises(ValueError):
        MLPPolicy.from_module(torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)))
