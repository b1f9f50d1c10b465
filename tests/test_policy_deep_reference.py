"""DeepMLPPolicy.__call__ (torch float64: what the per-step path of datasets.collect runs, and what the GPU tests hold the fused launch
to) against an independent restatement of emei_rollout_policy_deep's normative arithmetic: numpy float64 scalars in explicit Python
loops, one multiply and one add per term in ascending index order, the two hidden layers rounded to float32 before their ReLUs.  Bit
for bit under out="clip" and on a discrete binding, NaN and +-inf inputs included.  Plus the host logic around it: the shape checks,
MLPPolicy.from_module's sequences, DeepPolicyPopulation's stacking and views."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from emei_amd import _lib  # noqa: E402
from emei_amd.policy import DeepMLPPolicy, DeepPolicyPopulation, MLPPolicy, PolicyPopulation  # noqa: E402


def _relu32(z):
    h = np.float32(z)
    return np.float64(h) if h > np.float32(0) else np.float64(0.0)  # NaN > 0 is false: NaN gives 0


def deep_reference(w, x, lo, hi, discrete):
    """the header's clause, entry by entry; w = (w1, b1, w2, b2, w3, b3) float32 arrays, x [N, obs_dim] float32"""
    w1, b1, w2, b2, w3, b3 = w
    out = np.zeros((x.shape[0], w3.shape[0]), dtype=np.int64 if discrete else np.float32)
    with np.errstate(all="ignore"):
        for n in range(x.shape[0]):
            h1 = []
            for j in range(w1.shape[0]):
                z = np.float64(b1[j])
                for k in range(w1.shape[1]):
                    z = z + np.float64(w1[j, k]) * np.float64(x[n, k])
                h1.append(_relu32(z))
            h2 = []
            for i in range(w2.shape[0]):
                z = np.float64(b2[i])
                for j in range(w2.shape[1]):
                    z = z + np.float64(w2[i, j]) * h1[j]
                h2.append(_relu32(z))
            for q in range(w3.shape[0]):
                y = np.float64(b3[q])
                for i in range(w3.shape[1]):
                    y = y + np.float64(w3[q, i]) * h2[i]
                if discrete:
                    out[n, q] = 1 if y >= 0 else 0  # NaN gives 0
                else:
                    a = np.float32(y)
                    a = a if a >= np.float32(lo) else np.float32(lo)  # fmaxf(a, lo): NaN gives lo
                    out[n, q] = a if a <= np.float32(hi) else np.float32(hi)
    return out


def _weights(rng, obs_dim, h1, h2, n_out, scale=2.0):
    f = lambda *s: (rng.standard_normal(s) * scale / np.sqrt(s[-1])).astype(np.float32)
    return f(h1, obs_dim), f(h1), f(h2, h1), f(h2), f(n_out, h2), f(n_out)


def _policy(w, out="clip"):
    w1, b1, w2, b2, w3, b3 = w
    return DeepMLPPolicy(w3, b3, w2, b2, w1, b1, out=out)


@pytest.mark.parametrize("h1,h2", [(1, 1), (5, 3), (64, 33)])
@pytest.mark.parametrize("obs_dim,n_out,discrete,lo,hi", [(4, 1, True, -1.0, 1.0), (4, 1, False, -3.0, 3.0), (17, 6, False, -1.0, 1.0)])
def test_call_is_the_normative_arithmetic(h1, h2, obs_dim, n_out, discrete, lo, hi):
    rng = np.random.default_rng(1000 * h1 + 10 * h2 + obs_dim)
    w = _weights(rng, obs_dim, h1, h2, n_out)
    N = 24 if h1 == 64 else 70
    x = rng.standard_normal((N, obs_dim)).astype(np.float32)
    x[1, 0], x[2, 1], x[3, 2], x[4, :] = np.nan, np.inf, -np.inf, np.nan
    pol = _policy(w)
    pol.discrete, pol.lo, pol.hi = discrete, lo, hi
    got = pol(torch.as_tensor(x)).numpy()
    want = deep_reference(w, x, lo, hi, discrete)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want if n_out > 1 else want[:, 0])
    if not discrete and h1 > 1:
        assert (np.abs(want[5:]) < hi).any()  # not every row sits on the clip


def test_special_values():
    nan, inf = np.float32("nan"), np.float32("inf")
    one = lambda *v: np.float32(v)
    # obs_dim 1, widths (2, 2), one output: h1 = relu((x, -x)), h2 = relu((h1_0 - h1_1 + 1, h1_1)), y = h2_0 + 2 h2_1 + 0.25
    w = (one([1], [-1]), one(0, 0), one([1, -1], [0, 1]), one(1, 0), one([1, 2]), one(0.25))
    pol = _policy(w)
    pol.discrete, pol.lo, pol.hi = False, -3.0, 3.0
    x = one([0.5], [-0.5], [nan], [inf], [-inf])
    # 0.5: h1 = (0.5, 0), h2 = (1.5, 0), y = 1.75.  -0.5: h1 = (0, 0.5), h2 = (0.5, 0.5), y = 1.75.
    # NaN: both first-layer units are NaN -> 0, so h2 = (1, 0) and y = 1.25 (NaN into a ReLU gives 0).
    # +inf: h1 = (inf, 0), h2_0 = inf - 0 + 1 = inf, y = inf -> hi.  -inf: h1 = (0, inf), h2_0 = relu(-inf) = 0, h2_1 = inf -> hi.
    want = one(1.75, 1.75, 1.25, 3.0, 3.0)
    assert np.array_equal(pol(torch.as_tensor(x)).numpy(), want)
    assert np.array_equal(deep_reference(w, x, -3.0, 3.0, False)[:, 0], want)
    # NaN into the clip gives lo: an infinite output weight on a zero unit is inf * 0 = NaN
    wn = (one([1], [-1]), one(0, 0), one([1, 0], [0, 1]), one(0, 0), one([inf, 1]), one(0))
    pn = _policy(wn)
    pn.discrete, pn.lo, pn.hi = False, -3.0, 3.0
    assert np.array_equal(pn(torch.as_tensor(one([-2.0]))).numpy(), one(-3.0))
    pn.discrete = True
    assert np.array_equal(pn(torch.as_tensor(one([-2.0], [2.0]))).numpy(), [0, 1])  # NaN >= 0 is false; inf >= 0
    # each hidden layer is rounded to float32 before it is used
    third = np.float32(1 / 3)
    wr = (one([third]), one(0), one([third]), one(0), one([1]), one(0))
    pr = _policy(wr)
    pr.discrete, pr.lo, pr.hi = False, -3.0, 3.0
    h1 = np.float32(np.float64(third) * np.float64(third))
    h2 = np.float32(np.float64(third) * np.float64(h1))
    assert pr(torch.as_tensor(one([third]))).numpy()[0] == h2
    # tanh maps onto [lo, hi]
    pt = _policy((one([1]), one(0), one([1]), one(0), one([1]), one(0)), out="tanh")
    pt.discrete, pt.lo, pt.hi = False, -3.0, 3.0
    a = pt(torch.as_tensor(one([0], [40], [-40], [0.5]))).numpy()
    assert a[0] == 0 and a[1] == 3.0 and a[2] == 0 and a[3] == np.float32(3.0 * np.tanh(0.5))


def test_shape_checks_and_struct():
    rng = np.random.default_rng(3)
    w1, b1, w2, b2, w3, b3 = _weights(rng, 17, 5, 3, 6)
    pol = DeepMLPPolicy(w3, b3, w2, b2, w1, b1, out="tanh")
    assert isinstance(pol, MLPPolicy)
    assert (pol.hidden1, pol.hidden2, pol.obs_dim, pol.n_out, pol.out) == (5, 3, 17, 6, "tanh")
    assert pol.hidden == 3  # what the output layer, and a log-std head, read
    s = pol.struct()
    assert isinstance(s, _lib.EmeiPolicyDeep)
    assert (s.struct_size, s.hidden1, s.hidden2, s.out_mode, s.reserved) == (72, 5, 3, _lib.POLICY_OUT_TANH, 0)
    assert (s.w1, s.b1, s.w2, s.b2, s.w3, s.b3) == tuple(getattr(pol, k).data_ptr() for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    assert all(getattr(pol, k).dtype == torch.float32 and getattr(pol, k).is_contiguous() for k in DeepMLPPolicy._WEIGHTS)
    with pytest.raises(ValueError, match="hidden1"):
        DeepMLPPolicy(w3, b3, w2[:, :4], b2, w1, b1)
    with pytest.raises(ValueError, match="hidden2"):
        DeepMLPPolicy(w3[:, :2], b3, w2, b2, w1, b1)
    with pytest.raises(ValueError, match="b1"):
        DeepMLPPolicy(w3, b3, w2, b2, w1, b1[:4])
    with pytest.raises(ValueError, match="out"):
        DeepMLPPolicy(w3, b3, w2, b2, w1, b1, out="sigmoid")
    big = np.zeros((257, 4), np.float32)
    with pytest.raises(ValueError, match="hidden1=257"):
        DeepMLPPolicy(np.zeros((1, 2), np.float32), np.zeros(1, np.float32), np.zeros((2, 257), np.float32), np.zeros(2, np.float32), big,
                      np.zeros(257, np.float32))
    with pytest.raises(ValueError, match="hidden2=257"):
        DeepMLPPolicy(np.zeros((1, 257), np.float32), np.zeros(1, np.float32), np.zeros((257, 2), np.float32), np.zeros(257, np.float32),
                      np.zeros((2, 4), np.float32), np.zeros(2, np.float32))
    assert DeepMLPPolicy(np.zeros((1, 256), np.float32), np.zeros(1, np.float32), np.zeros((256, 256), np.float32), np.zeros(256, np.float32),
                         np.zeros((256, 4), np.float32), np.zeros(256, np.float32)).hidden1 == 256
    with pytest.raises(ValueError, match="bind"):
        pol(torch.zeros(2, 17))
    eng = type("E", (), dict(env_name="HalfCheetahRunning", act_dim=6, obs_dim=17, device=torch.device("cpu")))()
    assert pol.bind(eng).discrete is False and (pol.lo, pol.hi) == (-1.0, 1.0)
    with pytest.raises(ValueError, match="obs_dim=11"):
        pol.bind(type("E", (), dict(env_name="HopperRunning", act_dim=3, obs_dim=11, device=torch.device("cpu")))())


def test_from_module():
    lin, relu, tanh = torch.nn.Linear, torch.nn.ReLU, torch.nn.Tanh
    seq = torch.nn.Sequential(lin(17, 8), relu(), lin(8, 5), relu(), lin(5, 6), tanh())
    pol = MLPPolicy.from_module(seq)
    assert type(pol) is DeepMLPPolicy and (pol.out, pol.hidden1, pol.hidden2, pol.obs_dim, pol.n_out) == ("tanh", 8, 5, 17, 6)
    assert torch.equal(pol.w1, seq[0].weight.detach()) and torch.equal(pol.b2, seq[2].bias.detach()) and torch.equal(pol.w3, seq[4].weight.detach())
    module = torch.nn.Sequential(lin(4, 3), relu(), lin(3, 2), relu(), lin(2, 1))
    pol = MLPPolicy.from_module(module)
    assert type(pol) is DeepMLPPolicy and pol.out == "clip"
    assert type(DeepMLPPolicy.from_module(module)) is DeepMLPPolicy
    # the policy computes what the module computes (float32 module against float64 sums: a loose comparison of the wiring)
    pol.discrete, pol.lo, pol.hi = False, -1.0, 1.0
    x = torch.randn(9, 4, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.allclose(pol(x), torch.clamp(module(x), -1, 1)[:, 0], atol=1e-5)
    # what it took before, it takes as before
    one = MLPPolicy.from_module(torch.nn.Sequential(lin(4, 8), relu(), lin(8, 1), tanh()))
    assert type(one) is MLPPolicy and one.out == "tanh" and one.hidden == 8
    assert type(MLPPolicy.from_module(torch.nn.Sequential(lin(17, 6)))) is MLPPolicy
    for bad in ((lin(4, 8), tanh(), lin(8, 1)), (lin(4, 8), relu(), lin(8, 8), tanh(), lin(8, 1)), (lin(4, 8), relu(), lin(8, 8), relu()),
                (lin(4, 8), relu(), lin(8, 8), relu(), lin(8, 8), relu(), lin(8, 1)), (lin(4, 8), lin(8, 8), lin(8, 1)), ()):
        with pytest.raises(ValueError, match="from_module"):
            MLPPolicy.from_module(torch.nn.Sequential(*bad))
    with pytest.raises(ValueError, match="bias"):
        MLPPolicy.from_module(torch.nn.Sequential(lin(4, 3), relu(), lin(3, 2, bias=False), relu(), lin(2, 1)))


def test_population_stacking_and_views():
    rng = np.random.default_rng(5)
    members = [_policy(_weights(rng, 4, 5, 3, 1)) for _ in range(3)]
    pop = DeepPolicyPopulation.from_policies(members)
    assert len(pop) == 3 and (pop.hidden1, pop.hidden2, pop.obs_dim, pop.n_out) == (5, 3, 4, 1)
    assert tuple(pop.w1.shape) == (3, 5, 4) and tuple(pop.b1.shape) == (3, 5) and tuple(pop.w2.shape) == (3, 3, 5)
    assert tuple(pop.b2.shape) == (3, 3) and tuple(pop.w3.shape) == (3, 1, 3) and tuple(pop.b3.shape) == (3, 1)
    s = pop.struct()
    assert isinstance(s, _lib.EmeiPolicyDeep) and (s.struct_size, s.hidden1, s.hidden2, s.reserved) == (72, 5, 3, 0)
    assert s.w2 == pop.w2.data_ptr() and s.b3 == pop.b3.data_ptr()
    for p in (0, 1, 2, -1):
        view = pop[p]
        assert type(view) is DeepMLPPolicy
        for k in DeepMLPPolicy._WEIGHTS:
            assert torch.equal(getattr(view, k), getattr(members[p], k))
        # a view, at member p's offset behind the base pointer: the layout the kernels index
        q = p % 3
        assert view.w2.data_ptr() == pop.w2.data_ptr() + q * 3 * 5 * 4 and view.b1.data_ptr() == pop.b1.data_ptr() + q * 5 * 4
    with pytest.raises(IndexError):
        pop[3]
    with pytest.raises(ValueError, match="non-empty"):
        DeepPolicyPopulation.from_policies([])
    one_layer = MLPPolicy(np.zeros((1, 5), np.float32), np.zeros(1, np.float32), np.zeros((5, 4), np.float32), np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="DeepMLPPolicy"):
        DeepPolicyPopulation.from_policies([members[0], one_layer])
    with pytest.raises(ValueError, match="DeepPolicyPopulation"):
        PolicyPopulation.from_policies([members[0]])
    with pytest.raises(ValueError, match="w2"):
        DeepPolicyPopulation.from_policies([members[0], _policy(_weights(rng, 4, 5, 2, 1))])
    with pytest.raises(ValueError, match="out="):
        DeepPolicyPopulation.from_policies([members[0], _policy(_weights(rng, 4, 5, 3, 1), out="tanh")])
    with pytest.raises(ValueError, match="hidden1"):
        DeepPolicyPopulation(pop.w3, pop.b3, pop.w2[:, :, :4], pop.b2, pop.w1, pop.b1)
    eng = type("E", (), dict(env_name="CartPoleSwingUp", act_dim=0, obs_dim=4, device=torch.device("cpu")))()
    assert pop.bind(eng)[1].discrete is True
    import emei_amd

    assert emei_amd.DeepMLPPolicy is DeepMLPPolicy and emei_amd.DeepPolicyPopulation is DeepPolicyPopulation
