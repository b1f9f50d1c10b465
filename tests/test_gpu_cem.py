"""emei_plan_cem / emei_sample_candidates_sigma on the GPU (Engine.plan_cem / HipEnv.plan_cem / Engine.sample_candidates(sigma=tensor)).

The yardstick is the definition, as in tests/test_gpu_mppi.py: for the candidates emei_sample_candidates writes out and the returns
emei_evaluate_sequences gives them (both tied to the specification and to the CPU oracle by their own tests), the NumPy restatement
of tests/cem_reference.py — the planner's order as an explicit comparator, the moments in float64.

Tolerances.  The kernel and the reference differ in float64 summation order and one sqrt only.  mean_out: that can move the one final
rounding to float32 by at most one float32 step — one spacing at max(|lo|, |hi|) of the env's range (test_gpu_mppi._step_tol's rule).
std_out: one float32 spacing at hi - lo, the largest value a standard deviation inside the range could be rounded at, plus the
summation error of S2 / M (K * 2^-52 relative) carried through the square root, d sqrt(v) = dv / (2 sqrt(v)) <= K * 2^-52 * (S2 / M) /
std, from the reference's own float64 values.  best_index / best_return / elite_return and the elite SET (read back from the
workspace, where the finish kernel leaves the 0 / 1 membership) are exact."""
import numpy as np
import pytest

import cem_reference as C
from conftest import rel_err
from test_gpu_mppi import CH, OFFSET, _engine, _nominal, _range, _start, _step_tol

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TINY = float(np.finfo(np.float64).tiny)


def _sigma_map(eng, nom, seed):
    """a sigma per entry of `nom`: between 5 % and 50 % of the half range"""
    _, hi = _range(eng)
    rng = np.random.default_rng(seed)
    return torch.as_tensor((rng.uniform(0.05, 0.5, tuple(nom.shape)) * hi).astype(np.float32), device=eng.device)


def _members(eng, K):
    """the elite set of the last plan_cem call: the workspace holds emei_plan_shooting's 16-byte records, one per (wave, env) segment
    bound, then one float64 per candidate, which the finish kernel overwrites with the 0 / 1 membership (abi.hip)"""
    nk = eng.n_envs * K
    off = 2 * ((nk + 63) // 64 + eng.n_envs)
    return eng._cem_ws[off:off + nk].view(eng.n_envs, K).cpu().numpy() != 0


def _same(a, b):
    """bit-equal as far as the order sees values: NaN equals NaN, and the sign of a zero counts"""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def _check_definition(eng, H, K, M, seed, gamma, nominal=None, sigma=None, start_state=None, cheetah=False, out=None, out_sigma=None,
                      label=""):
    """plan_cem against cem_reference on (sample_candidates, evaluate_sequences) -> (cand, ret, reference, outputs) as NumPy"""
    N = eng.n_envs
    is_map = isinstance(sigma, torch.Tensor)
    cand = eng.sample_candidates(H, K, seed, nominal=nominal, sigma=sigma)
    ret, _ = eng.evaluate_sequences(cand, discount=gamma, start_state=start_state)
    cand, ret = cand.cpu().numpy(), ret.cpu().numpy()
    lo, hi = _range(eng)
    with np.errstate(all="ignore"):
        want = C.cem(cand, ret, M, nominal=None if nominal is None else nominal.cpu().numpy(),
                     lo=None if eng.act_dim == 0 else lo, hi=None if eng.act_dim == 0 else hi)
    if not is_map:  # the winner is emei_plan_shooting's, bit for bit
        _, sret, sidx = eng.plan_shooting(H, K, seed, discount=gamma, nominal=nominal, sigma=sigma, start_state=start_state)
    got = eng.plan_cem(H, K, M, seed, discount=gamma, nominal=nominal, sigma=sigma, start_state=start_state, out=out,
                       out_sigma=out_sigma, elite_return=True)
    mean, std, bret, idx, er = got
    members = _members(eng, K)
    tail = (eng.act_dim,) if eng.act_dim > 1 else ()
    assert mean.dtype == torch.float32 and bret.dtype == torch.float64 and idx.dtype == torch.int32 and er.dtype == torch.float64
    shape = (H, N) + tail if nominal is None else tuple(nominal.shape)
    assert tuple(mean.shape) == shape and tuple(bret.shape) == (N,) and tuple(idx.shape) == (N,) and tuple(er.shape) == (N,)
    assert (std is None) == (eng.act_dim == 0)
    if std is not None:
        assert std.dtype == torch.float32 and tuple(std.shape) == shape
    if not is_map:
        assert torch.equal(idx, sidx) and np.array_equal(bret.cpu().numpy(), sret.cpu().numpy(), equal_nan=True)
    mean, bret, idx, er = (x.cpu().numpy() for x in (mean, bret, idx, er))
    std = None if std is None else std.cpu().numpy()
    if cheetah:
        # r_k may differ from the composition's by 1e-9 relative (the constraint-slot lending), which could carry a
        # candidate across the threshold: the case must keep its M-th and (M + 1)-th returns further apart than that, in EVERY env
        srt = -np.sort(-ret, axis=1)
        if M < K:
            gap = srt[:, M - 1] - srt[:, M]
            print(f"{label}: gaps at the threshold {gap} against {1e-6 * np.maximum(np.abs(srt[:, M - 1]), 1e-3)}")
            assert (gap > 1e-6 * np.maximum(np.abs(srt[:, M - 1]), 1e-3)).all(), "precondition: choose another seed"
        assert rel_err(bret, want.best_return) <= 1e-9 and rel_err(er, want.elite_return) <= 1e-9
        best = ret.max(1)
        assert (np.abs(ret[np.arange(N), idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
    else:
        assert np.array_equal(idx, want.best_index) and _same(bret, want.best_return) and _same(er, want.elite_return)
    assert (members.sum(1) == M).all() and np.array_equal(members, want.members)
    tol = _step_tol(eng)
    err = np.abs(mean.astype(np.float64) - want.mean.astype(np.float64)).max()
    msg = f"{label or eng.env_name} N={N} K={K} M={M} H={H}: max |mean_out - reference| = {err:.3e} (bound {tol:.3e})"
    assert np.isfinite(mean).all()
    if std is not None:
        sbound = float(np.spacing(np.float32(hi - lo))) + K * 2.0 ** -52 * want.s2_over_m / np.maximum(want.std64, TINY)
        serr = np.abs(std.astype(np.float64) - want.std.astype(np.float64))
        worst = np.unravel_index(np.argmax(serr - sbound), serr.shape)
        msg += (f", max |std_out - reference| = {serr.max():.3e} (bound {sbound.min():.3e} .. {sbound.max():.3e}; at the entry closest "
                f"to its bound {serr[worst]:.3e} against {sbound[worst]:.3e}), reference std {want.std64.min():.3g} .. {want.std64.max():.3g}")
        print(msg)
        assert np.isfinite(std).all() and (std >= 0).all()
        assert (serr <= sbound).all()
    else:
        print(msg)
    assert err <= tol
    plo, phi = (0.0, 1.0) if eng.act_dim == 0 else (lo, hi)
    assert mean.min() >= plo and mean.max() <= phi
    return cand, ret, want, (mean, std, bret, idx, er, members)


# ------------------------------------------------------------------------------------------------ a. the definition
# (env, engine kwargs, N, K, M, H, discount, start_state, candidates): (5, 13, 4) has envs that straddle waves of the first launch,
# (64, 64, 8) is whole waves, (3, 300, 37) on integer returns ties heavily exactly at the threshold and gives lanes several
# candidates, (1, 257, 257) / (1, 257, 1) / (257, 1, 1) are M = K, M = 1, K = 1, (2, 4100, 512) gives a lane more than 64 rows; the
# Hopper's 15 words leave the last Box-Muller pair half used and put components astride Philox blocks.
# candidates: None = fair coins / uniform, "scalar" = a nominal with one sigma, "map" = a nominal with a sigma per entry
CASES = [
    ("CartPoleSwingUp", dict(precision="ref", env_index_offset=OFFSET), 5, 13, 4, 9, 0.99, False, None),
    ("CartPoleSwingUp", dict(precision="f32", freq_rate=2), 64, 64, 8, 40, 0.99, True, "scalar"),
    ("CartPoleBalancing", dict(), 3, 300, 37, 50, 1.0, False, None),
    ("CartPoleSwingUp", dict(env_index_offset=OFFSET), 1, 257, 257, 5, 0.99, False, "scalar"),
    ("CartPoleSwingUp", dict(env_index_offset=OFFSET), 1, 257, 1, 5, 0.99, False, "scalar"),
    ("CartPoleSwingUp", dict(), 257, 1, 1, 5, 1.0, False, None),
    ("CartPoleSwingUp", dict(), 2, 4100, 512, 5, 0.99, False, None),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 4, 5, 0.99, False, None),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 4, 5, 0.99, True, "scalar"),
    ("ReboundInvertedPendulumBalancing", dict(precision="ref"), 5, 13, 4, 5, 0.99, True, "map"),
    ("ReboundInvertedDoublePendulumBalancing", dict(), 3, 300, 37, 7, 0.99, False, "map"),
    ("HopperRunning", dict(**CH), 5, 13, 4, 5, 0.99, True, "map"),
    ("HalfCheetahRunning", dict(**CH), 5, 13, 4, 3, 0.99, False, "scalar"),
]


@pytest.mark.parametrize("name,kw,N,K,M,H,gamma,start,mode", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_update_equals_its_definition(name, kw, N, K, M, H, gamma, start, mode):
    kw = dict(kw)
    kw.setdefault("env_index_offset", 3)
    eng = _engine(name, N, **kw)
    eng.reset(seed=21 + N)
    st = _start(eng) if start else None
    nom, sigma = _nominal(eng, H, seed=K) if mode else (None, None)
    if mode == "map":
        sigma = _sigma_map(eng, nom, seed=K + 1)
    cand, ret, want, (mean, std, bret, idx, er, members) = _check_definition(
        eng, H, K, M, 1000 * N + K, gamma, nominal=nom, sigma=sigma, start_state=st, cheetah=name == "HalfCheetahRunning")
    c64 = cand.astype(np.float64)
    if M == 1:
        assert np.array_equal(er, bret, equal_nan=True)
        picked = np.stack([cand[:, i, idx[i]] for i in range(N)], axis=1).astype(np.float32).reshape(mean.shape)
        assert np.abs(mean - picked).max() <= _step_tol(eng)
    if M == K and eng.act_dim == 0:
        assert np.abs(mean - c64.mean(2)).max() <= _step_tol(eng)
    if name == "CartPoleBalancing":
        # integer returns: the threshold value is shared by candidates on both sides of the cut, which k alone separates
        tied_out = ((ret == er[:, None]) & ~members).sum(1)
        print(f"candidates tied with the threshold and left out, per env: {tied_out}")
        assert (tied_out > 0).any()
        for i in range(N):
            ks_in, ks_out = np.nonzero((ret[i] == er[i]) & members[i])[0], np.nonzero((ret[i] == er[i]) & ~members[i])[0]
            assert len(ks_out) == 0 or ks_in.max() < ks_out.min()
    if eng.act_dim == 0 and 1 < M:
        assert ((mean > 0) & (mean < 1)).any()  # probabilities, not copies of one candidate
    assert eng.solver_cap_hits() == 0


# ------------------------------------------------------------------------------------------------ b. special values
def test_odd_start_rows():
    """NaN, +-inf, beyond-threshold and on-threshold start rows mixed with ordinary ones inside one wave (the rows
    tests/test_gpu_plan.py sends through the same kernels), plus two rows that are NaN throughout"""
    from test_gpu_plan import _odd_rows

    name, N, K, M, H, gamma = "CartPoleSwingUp", 70, 3, 2, 12, 0.95
    plain, rows, odd = _odd_rows(name, np.random.default_rng(5), N)
    rows[[3, 64]] = np.nan  # every coordinate: in the first wave and at the start of the second
    odd = np.union1d(odd, [3, 64])
    eng = _engine(name, N)
    eng.reset(seed=1)
    cand, ret, want, (mean, std, bret, idx, er, members) = _check_definition(
        eng, H, K, M, 9, gamma, start_state=torch.as_tensor(rows, device=eng.device), label="odd rows")
    nan = np.isnan(ret)
    all_nan = nan.all(1)
    assert all_nan[[3, 64]].all()  # the reward is (cos theta + 1) / 2: a NaN row has NaN returns
    # NaN-return candidates are members only where fewer than M others exist
    assert ((members & nan).sum(1) == np.maximum(M - (~nan).sum(1), 0)).all()
    assert np.isnan(er[(~nan).sum(1) < M]).all() and not np.isnan(er[(~nan).sum(1) >= M]).any()
    # all-NaN envs: the first M candidates by k, k* = 0, a NaN return
    first = cand[:, :, :M].astype(np.float64).mean(2)
    assert members[all_nan][:, :M].all() and np.abs(mean[:, all_nan] - first[:, all_nan]).max() <= _step_tol(eng)
    assert (idx[all_nan] == 0).all() and np.isnan(bret[all_nan]).all()
    assert not np.isnan(bret[~all_nan]).any() and np.isfinite(mean).all()
    # the ordinary envs of the same waves: the bits of a run without the odd neighbours
    _, _, _, (mean0, _, bret0, idx0, er0, members0) = _check_definition(
        eng, H, K, M, 9, gamma, start_state=torch.as_tensor(plain, device=eng.device), label="plain rows")
    keep = np.setdiff1d(np.arange(N), odd)
    assert np.array_equal(mean[:, keep], mean0[:, keep]) and np.array_equal(er[keep], er0[keep])
    assert np.array_equal(members[keep], members0[keep])
    assert np.array_equal(idx[keep], idx0[keep]) and np.array_equal(bret[keep], bret0[keep]) and np.isfinite(bret0).all()


# ------------------------------------------------------------------------------------------------ c. the sigma map
@pytest.mark.parametrize("name,kw", [("ReboundInvertedPendulumSwingUp", dict()), ("HopperRunning", dict(CH))])
def test_sigma_map(name, kw):
    N, K, M, H = 5, 13, 4, 5
    eng = _engine(name, N, env_index_offset=OFFSET, **kw)
    eng.reset(seed=2)
    nom, s = _nominal(eng, H, seed=3)
    # a map filled with s is the scalar s
    full = torch.full_like(nom, s)
    assert torch.equal(eng.sample_candidates(H, K, 17, nominal=nom, sigma=full), eng.sample_candidates(H, K, 17, nominal=nom, sigma=s))
    a = eng.plan_cem(H, K, M, 17, discount=0.99, nominal=nom, sigma=full, elite_return=True)
    b = eng.plan_cem(H, K, M, 17, discount=0.99, nominal=nom, sigma=s, elite_return=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # zeros in some entries: the (clipped) mean itself — the nominal lies inside the range — and a standard deviation of exactly 0
    smap = _sigma_map(eng, nom, seed=4)
    zero = torch.as_tensor(np.random.default_rng(5).random(tuple(nom.shape)) < 0.3, device=eng.device)
    smap[zero] = 0.0
    cand = eng.sample_candidates(H, K, 18, nominal=nom, sigma=smap)
    cz = cand.reshape(nom.shape[:2] + (K,) + tuple(nom.shape[2:]))
    zb = zero.unsqueeze(2).expand_as(cz)
    assert torch.equal(cz[zb], nom.unsqueeze(2).expand_as(cz)[zb]) and bool(zero.any()) and not bool(zero.all())
    _, _, _, (mean, std, *_) = _check_definition(eng, H, K, M, 18, 0.99, nominal=nom, sigma=smap, label=f"{name} sigma_map with zeros")
    z = zero.cpu().numpy()
    assert np.array_equal(mean[z], nom.cpu().numpy()[z]) and (std[z] == 0).all() and (std[~z] > 0).any()
    assert eng.solver_cap_hits() == 0


# ------------------------------------------------------------------------------------------------ d. shard invariance
@pytest.mark.parametrize("name,kw,mode", [("CartPoleSwingUp", dict(), "scalar"), ("HopperRunning", dict(CH), "map"),
                                          ("ReboundInvertedPendulumSwingUp", dict(), None)])
def test_shards_give_the_whole(name, kw, mode):
    N, K, M, H = 192, 24, 5, 15
    whole = _engine(name, N, env_index_offset=0, **kw)
    parts = [_engine(name, 64, env_index_offset=o, **kw) for o in (0, 64, 128)]
    whole.reset(seed=6)
    st = whole.get_state()
    nom, sigma = _nominal(whole, H, seed=1) if mode else (None, None)
    if mode == "map":
        sigma = _sigma_map(whole, nom, seed=2)
    want = whole.plan_cem(H, K, M, 99, discount=0.97, nominal=nom, sigma=sigma, start_state=st, elite_return=True)
    got = []
    for p, o in zip(parts, (0, 64, 128)):
        sl = slice(o, o + 64)
        got.append(p.plan_cem(H, K, M, 99, discount=0.97, nominal=None if nom is None else nom[:, sl].contiguous(),
                              sigma=sigma[:, sl].contiguous() if isinstance(sigma, torch.Tensor) else sigma,
                              start_state=st[sl].contiguous(), elite_return=True))
    for q, w in enumerate(want):
        if w is None:
            assert all(g[q] is None for g in got)
            continue
        cat = torch.cat([g[q] for g in got], dim=1 if q < 2 else 0)
        assert torch.equal(cat, w), q
    assert not torch.equal(want[0][:, :64], want[0][:, 64:128])  # the shards do not simply repeat each other


# ------------------------------------------------------------------------------------------------ e. in place
@pytest.mark.parametrize("name,kw,N,K,M,H", [("CartPoleSwingUp", dict(), 70, 100, 9, 21), ("HopperRunning", dict(CH), 5, 13, 4, 5),
                                             ("ReboundInvertedPendulumSwingUp", dict(), 64, 64, 8, 10)])
def test_in_place_equals_out_of_place(name, kw, N, K, M, H):
    eng = _engine(name, N, **kw)
    eng.reset(seed=3)
    nom, sigma = _nominal(eng, H, seed=2)
    if eng.act_dim > 0:
        sigma = _sigma_map(eng, nom, seed=3)
    keep, keep_s = nom.clone(), None if sigma is None else sigma.clone()
    want = eng.plan_cem(H, K, M, 5, discount=0.99, nominal=nom, sigma=sigma, elite_return=True)
    assert torch.equal(nom, keep) and want[0].data_ptr() != nom.data_ptr()
    assert sigma is None or (torch.equal(sigma, keep_s) and want[1].data_ptr() != sigma.data_ptr())
    other, other_s = torch.full_like(nom, 7.0), None if sigma is None else torch.full_like(nom, 7.0)
    got = eng.plan_cem(H, K, M, 5, discount=0.99, nominal=nom, sigma=sigma, out=other, out_sigma=other_s, elite_return=True)
    assert got[0] is other and got[1] is other_s and torch.equal(nom, keep)
    for x, y in zip(got, want):
        assert (x is None and y is None) or torch.equal(x, y)
    got = eng.plan_cem(H, K, M, 5, discount=0.99, nominal=nom, sigma=sigma, out=nom, out_sigma=sigma, elite_return=True)
    assert got[0] is nom and got[1] is sigma
    for x, y in zip(got, want):
        assert (x is None and y is None) or torch.equal(x, y)
    assert not torch.equal(nom, keep) and (sigma is None or not torch.equal(sigma, keep_s))


# ------------------------------------------------------------------------------------------------ f. the contract
def test_repeat_calls_give_the_same_bits():
    eng = _engine("HopperRunning", 37, **CH)
    eng.reset(seed=4)
    nom, _ = _nominal(eng, 6, seed=3)
    smap = _sigma_map(eng, nom, seed=4)
    a = eng.plan_cem(6, 70, 9, 11, discount=0.99, nominal=nom, sigma=smap, elite_return=True)
    eng.plan_cem(3, 200, 200, 12)  # another shape through the same workspace in between
    b = eng.plan_cem(6, 70, 9, 11, discount=0.99, nominal=nom, sigma=smap, elite_return=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert eng.solver_cap_hits() == 0


@pytest.mark.parametrize("name,kw", [("CartPoleSwingUp", dict(max_episode_steps=9)), ("HopperRunning", dict(max_episode_steps=6, **CH))])
def test_handle_untouched(name, kw):
    N = 96
    a, b = _engine(name, N, seed=4, **kw), _engine(name, N, seed=4, **kw)
    g = torch.Generator(device=a.device).manual_seed(9)
    step_acts = torch.randint(0, 2, (20, N), generator=g, device=a.device, dtype=torch.uint8) if a.act_dim == 0 \
        else torch.rand((20, N, a.act_dim), generator=g, device=a.device) * 2 - 1
    for e in (a, b):
        e.reset(seed=4)
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    a.plan_cem(15, 5, 2, 123, discount=0.9, elite_return=True)
    assert torch.equal(a.get_state(), b.get_state())
    for x, y in zip(a.get_counters(), b.get_counters()):
        assert torch.equal(x, y)
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]  # auto-reset: the reset key is the handle's own still
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.unfreeze()
    assert torch.equal(a.get_state(), b.get_state())
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_capture_replays_the_same_result():
    N, K, M, H = 256, 16, 3, 50
    eng = _engine("CartPoleSwingUp", N)
    eng.reset(seed=8)
    nom, _ = _nominal(eng, H, seed=4)
    want = eng.plan_cem(H, K, M, 31, discount=0.99, nominal=nom, elite_return=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # one linear chain: plan, finish
        got = eng.plan_cem(H, K, M, 31, discount=0.99, nominal=nom, elite_return=True)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in got:
            if x is not None:
                x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert (x is None and y is None) or torch.equal(x, y)


def test_argument_checks_on_a_handle():
    import ctypes as ct

    from emei_amd import _lib as L

    eng = _engine("HopperRunning", 4)
    with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet
        eng.plan_cem(3, 4, 2, 0)
    eng.reset(seed=0)
    good = torch.zeros((3, 4, 3), device=eng.device)
    eng.plan_cem(3, 4, 2, 0, nominal=good, sigma=0.1)
    eng.plan_cem(3, 4, 2, 0, nominal=good, sigma=torch.full_like(good, 0.1))
    mean, std, ret, idx = eng.plan_cem(3, 4, 2, 0)
    assert tuple(mean.shape) == (3, 4, 3) and mean.dtype == torch.float32 and tuple(std.shape) == (3, 4, 3)
    for bad in (dict(nominal=good[:2].contiguous(), sigma=0.1), dict(nominal=good.double(), sigma=0.1), dict(nominal=good.cpu(), sigma=0.1),
                dict(nominal=good), dict(nominal=good, sigma=0.0), dict(nominal=good, sigma=float("nan")), dict(discount=0.0),
                dict(sigma=torch.full_like(good, 0.1)), dict(nominal=good, sigma=torch.full_like(good, 0.1)[:2].contiguous()),
                dict(nominal=good, sigma=torch.full_like(good, 0.1).double()), dict(nominal=good, sigma=torch.full_like(good, 0.1).cpu()),
                dict(out=good[:2].contiguous()), dict(out=good.double()), dict(out_sigma=good[:2].contiguous()), dict(out_sigma=good.cpu()),
                dict(start_state=torch.zeros(4, eng.state_dim, device=eng.device))):
        with pytest.raises(ValueError):
            eng.plan_cem(3, 4, 2, 0, **bad)
    for m in (0, -1, 5):
        with pytest.raises(ValueError, match="n_elites"):
            eng.plan_cem(3, 4, m, 0)
    with pytest.raises(ValueError):
        eng.plan_cem(0, 4, 2, 0)
    with pytest.raises(ValueError):
        eng.sample_candidates(3, 4, 0, sigma=torch.full_like(good, 0.1))  # a map needs a nominal
    # the ABI's own refusals behind the binding's: raw calls on live handles, nothing launched
    lib = L.lib()
    buf = {k: torch.zeros(64, dtype=torch.float64, device=eng.device) for k in ("ws", "mean", "std", "nom", "smap", "out")}
    p = {k: ct.c_void_p(v.data_ptr()) for k, v in buf.items()}

    def cem(h, nominal=None, smap=None, ws=p["ws"], mean=p["mean"], std=None, m=2):
        rc = lib.emei_plan_cem(h, 3, 4, m, 0, nominal, 0.1, smap, 1.0, None, ws, mean, std, None, None, None, None)
        return rc, lib.emei_last_error().decode()

    for kw in (dict(smap=p["smap"]), dict(ws=None), dict(mean=None), dict(m=5)):
        rc, msg = cem(eng._h, **kw)
        assert rc == L.ERR_INVALID and msg.startswith("emei_plan_cem:"), (kw, rc, msg)
    assert cem(eng._h, nominal=p["nom"], smap=p["smap"], std=p["std"])[0] == L.OK
    cart = _engine("CartPoleSwingUp", 4)
    cart.reset(seed=0)
    for kw in (dict(nominal=p["nom"], smap=p["smap"]), dict(std=p["std"])):
        rc, msg = cem(cart._h, **kw)
        assert rc == L.ERR_INVALID and "discrete" in msg, (kw, rc, msg)
    assert cem(cart._h, nominal=p["nom"])[0] == L.OK
    with pytest.raises(ValueError):
        cart.plan_cem(3, 4, 2, 0, nominal=torch.full((3, 4), 0.5, device=cart.device), sigma=torch.full((3, 4), 0.5, device=cart.device))
    with pytest.raises(ValueError):
        cart.plan_cem(3, 4, 2, 0, out_sigma=torch.zeros((3, 4), device=cart.device))
    for h, nominal, smap in ((cart._h, p["nom"], p["smap"]), (eng._h, None, p["smap"]), (eng._h, p["nom"], None)):
        dtype = 0 if h is cart._h else 3
        rc = lib.emei_sample_candidates_sigma(h, 3, 4, 0, nominal, smap, p["out"], dtype, None)
        assert rc == L.ERR_INVALID and lib.emei_last_error().decode().startswith("emei_sample_candidates_sigma:"), (nominal, smap)
    torch.cuda.synchronize()


def test_env_surface_numpy_and_tensor():
    import emei_amd

    env = emei_amd.make("CartPoleSwingUp-v0", num_envs=8)
    with pytest.raises(AssertionError):
        env.plan_cem(5, 4, 2, 0)
    env.reset(seed=0)
    prob, std, ret, idx = env.plan_cem(10, 16, 4, seed=3, discount=0.99, iterations=2)
    assert isinstance(prob, torch.Tensor) and prob.dtype == torch.float32 and tuple(prob.shape) == (10, 8) and std is None
    assert float(prob.min()) >= 0.0 and float(prob.max()) <= 1.0 and ret.dtype == torch.float64 and idx.dtype == torch.int32
    env.step((prob[0] >= 0.5).to(torch.int64))
    start = np.full((10, 8), 0.5, np.float32)
    out = env.plan_cem(10, 16, 4, seed=3, discount=0.99, nominal=start, elite_return=True)
    assert out[1] is None and all(isinstance(x, np.ndarray) for x in out if x is not None) and out[0].shape == (10, 8)
    assert out[4].dtype == np.float64 and (start == 0.5).all()
    hop = emei_amd.make("HopperRunning-v0", num_envs=4)
    hop.reset(seed=0)
    mean, std, ret, idx = hop.plan_cem(4, 8, 2, seed=1)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (4, 4, 3) and float(mean.abs().max()) <= 1.0
    assert tuple(std.shape) == (4, 4, 3) and float(std.min()) >= 0.0
    keep = mean.clone()
    again = hop.plan_cem(4, 8, 2, seed=2, nominal=mean, sigma=std.clamp_(min=0.05), iterations=2)
    assert torch.equal(mean, keep) and again[0] is not mean  # the caller's tensors are copied, not written
    with pytest.raises(ValueError):
        hop.plan_cem(4, 8, 2, seed=2, iterations=0)
    hop.step(again[0][0])


# ------------------------------------------------------------------------------------------------ g. iterations
@pytest.mark.parametrize("name,N,K,M,H", [("CartPoleSwingUp", 33, 40, 6, 12), ("HopperRunning", 5, 13, 4, 5),
                                          ("ReboundInvertedPendulumSwingUp", 5, 13, 4, 5)])
def test_iterations_are_chained_calls_and_each_equals_its_definition(name, N, K, M, H):
    """HipEnv.plan_cem(iterations=3) is three engine calls with the seeds seed, seed + 1, seed + 2, each taking the previous (mean,
    std) as its (nominal, sigma map); every link is held to the definition"""
    import emei_amd

    env = emei_amd.make(name + "-v0", num_envs=N)
    env.reset(seed=7)
    eng = env.engine
    sigma0 = None if eng.act_dim == 0 else 0.3
    nom0, _ = _nominal(eng, H, seed=5)
    got = env.plan_cem(H, K, M, 50, discount=0.99, nominal=nom0, sigma=sigma0, iterations=3, elite_return=True)
    nom, sigma = nom0.clone(), sigma0
    for it in range(3):
        _, _, _, (mean, std, bret, idx, er, _) = _check_definition(eng, H, K, M, 50 + it, 0.99, nominal=nom, sigma=sigma,
                                                                  label=f"{name} iteration {it}")
        nom = torch.as_tensor(mean, device=eng.device).contiguous()
        sigma = None if std is None else torch.as_tensor(std, device=eng.device).contiguous()
    for x, y in zip(got, (mean, std, bret, idx, er)):
        assert (x is None and y is None) or np.array_equal(x.cpu().numpy(), y, equal_nan=True)
    assert eng.solver_cap_hits() == 0


def test_iterating_does_not_lower_the_elite_threshold():
    """CartPoleSwingUp, four iterations from fair coins, the probabilities kept away from 0 and 1 by the caller as the README's loop
    does: the mean over the envs of the elite threshold (the M-th best return) of iteration 4 is not below iteration 1's"""
    N, K, M, H = 64, 64, 8, 30
    eng = _engine("CartPoleSwingUp", N)
    eng.reset(seed=12)
    prob, level = None, []
    for it in range(4):
        prob, _, _, _, er = eng.plan_cem(H, K, M, 700 + it, discount=0.99, nominal=prob, elite_return=True)
        prob.clamp_(0.05, 0.95)
        level.append(float(er.mean()))
    print(f"mean elite threshold per iteration: {level}")
    assert level[3] >= level[0]
