"""The terminal value of the open-loop planners on the GPU: Engine.evaluate_sequences / plan_shooting / plan_mppi / plan_cem with
value=DeepValueFunction (emei_evaluate_sequences_value, emei_plan_shooting_value, emei_plan_mppi_value, emei_plan_cem_value on
pend_plan_value_kernel / body_plan_value_kernel).

The yardstick is never the code under test: it is the plain evaluate_sequences plus the torch twin DeepValueFunction.__call__, both
pinned by their own tests.  For candidates `cand` (given, or written out by sample_candidates): ret, L, fobs =
evaluate_sequences(cand, final_obs=True); ended[i, k] = did any step of candidate k report the terminal bit, from replaying its
actions through rollout() from the start rows without auto-reset; the twin return is where(ended, ret, ret + g_H *
float64(value(fobs))) in NumPy float64, unfused, g_H by H multiplications (_g_H / _bootstrap of tests/test_gpu_policy_plan_deep.py).
Bounds: bit for bit everywhere except the HalfCheetah, which is held to the project's documented 1e-9 relative (the
constraint-slot lending); L and final_obs equal the plain call's exactly.  plan_mppi(value=) and plan_cem(value=) are held as
tests/test_gpu_mppi.py and tests/test_gpu_cem.py hold the plain calls — mppi_reference / cem_reference on the written-out candidates,
with their bounds — the bootstrapped twin returns in the place of evaluate_sequences' returns.

Shapes: (N = 3, K = 70) one env over two waves, (67, 5) segments astride wave edges with a ragged last wave, (1, 1); H in {1, 12};
value widths (9, 2), (3, 4), (1, 1); one (256, 256) case on CartPoleBalancing and HalfCheetahRunning for the 64 KiB tile and its
opt-in next to the cheetah's static LDS; env_index_offset = 2^32 + 7.  A case runs once and is shared by the tests that read it."""
import ctypes as C
import functools

import numpy as np
import pytest

import cem_reference as CR
import mppi_reference as MR
import policy_population_reference as PP
import shooting_reference as SR
from conftest import rel_err
from test_gpu_policy_plan_deep import CASES, OFFSET, _bits, _bootstrap, _engine, _g_H, _same, _value

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 2 ** 64 - 5  # the candidates' key
TINY = float(np.finfo(np.float64).tiny)
# (case, N, K, H, value widths, draws): draws None = fair coins / uniform on the ctrlrange; "nominal" = Bernoulli probabilities
# (discrete) or a Gaussian with a scalar sigma (continuous); "map" = as "nominal", and plan_cem draws with a sigma per entry
SHAPES = [
    ("cartpole-balancing", 3, 70, 12, (9, 2), None), ("cartpole-balancing", 67, 5, 12, (3, 4), None),
    ("cartpole-balancing", 67, 5, 1, (1, 1), "nominal"), ("cartpole-balancing", 1, 1, 1, (9, 2), None),
    ("cartpole-balancing", 67, 5, 12, (9, 2), "nominal"),  # Bernoulli probabilities per step: the nominal indexed at every t
    ("ip-boundary-balancing-rk4", 3, 70, 12, (3, 4), "map"), ("ip-boundary-balancing-rk4", 67, 5, 12, (9, 2), None),
    ("idp-ref", 3, 70, 12, (9, 2), None), ("idp-ref", 1, 1, 12, (3, 4), "nominal"), ("idp-f32", 67, 5, 12, (3, 4), "nominal"),
    ("idp-f32", 3, 70, 1, (1, 1), None),
    ("hopper-terminating", 3, 70, 12, (9, 2), "map"), ("hopper-terminating", 67, 5, 12, (3, 4), None),
    ("hopper-terminating", 67, 5, 12, (9, 2), "nominal"), ("hopper-terminating", 3, 70, 1, (1, 1), None),
    ("cheetah", 3, 70, 1, (9, 2), None), ("cheetah", 67, 5, 12, (3, 4), "nominal"),
]
IDS = ["%s-N%d-K%d-H%d-v%dx%d-%s" % (c, n, k, h, w[0], w[1], d or "plain-draws") for c, n, k, h, w, d in SHAPES]
ALL = pytest.mark.parametrize("case,N,K,H,widths,draws", SHAPES, ids=IDS)
# the cases whose (67, 5, 12) candidates were checked on the CPU oracle to hold both kinds, none undecidable at 1e-5
MIXED = {("cartpole-balancing", None), ("hopper-terminating", None), ("hopper-terminating", "nominal"), ("ip-boundary-balancing-rk4", None)}


def _start(eng, case):
    """host-built start rows where episodes should end inside H = 12: the CartPole's pole angle x 3, the Hopper's spread heights, the
    boundary pendulum's pole at +-(0.3 + 1.25 u) rad; elsewhere the reset state"""
    env = CASES[case]["env"]
    if case in ("idp-ref", "idp-f32", "cheetah"):
        return eng.get_state().clone().contiguous()
    rows = PP.gpu_start(env, eng.n_envs).copy()
    if env == "CartPoleBalancing":
        rows[:, 2] *= 3.0
    elif env == "BoundaryInvertedPendulumBalancing":
        u = np.random.default_rng(17).random((2, eng.n_envs))
        rows[:, 1] = np.where(u[0] < 0.5, -1.0, 1.0) * (0.3 + 1.25 * u[1])
    return torch.as_tensor(rows, device=eng.device, dtype=torch.float64).contiguous()


def _range(eng):
    if eng.act_dim == 0:
        return 0.0, 1.0
    return (-3.0, 3.0) if "InvertedPendulum" in eng.env_name and "Double" not in eng.env_name else (-1.0, 1.0)


def _step_tol(eng):
    lo, hi = _range(eng)
    return float(np.spacing(np.float32(max(abs(lo), abs(hi)))))


def _nominal(eng, H, draws, seed=3):
    """(nominal, sigma): None, None; Bernoulli probabilities; or means with a scalar sigma (the Hopper: mean 0, sigma 0.5)"""
    if draws is None:
        return None, None
    rng = np.random.default_rng(seed)
    N = eng.n_envs
    if eng.act_dim == 0:
        return torch.as_tensor(rng.uniform(0.1, 0.9, (H, N)).astype(np.float32), device=eng.device), None
    lo, hi = _range(eng)
    shape = (H, N, eng.act_dim) if eng.act_dim > 1 else (H, N)
    if eng.env_name == "HopperRunning":
        return torch.zeros(shape, dtype=torch.float32, device=eng.device), 0.5
    return torch.as_tensor(rng.uniform(0.5 * lo, 0.5 * hi, shape).astype(np.float32), device=eng.device), 0.4 * hi


def _sigma_map(eng, nom, seed=4):
    _, hi = _range(eng)
    rng = np.random.default_rng(seed)
    return torch.as_tensor((rng.uniform(0.05, 0.5, tuple(nom.shape)) * hi).astype(np.float32), device=eng.device)


def _ended(eng, cand, start):
    """[N, K] bool: did any step of candidate k report the terminal bit — its actions replayed through rollout() from the start
    rows, without auto-reset"""
    out = []
    for k in range(cand.shape[2]):
        eng.set_state(start)
        _, _, done = eng.rollout(cand[:, :, k].contiguous())
        out.append(((done & 1) != 0).any(dim=0))
    eng.set_state(start)
    return torch.stack(out, dim=1).cpu().numpy()


def _temperature(ret):
    sds = [np.std(r[np.isfinite(r)]) for r in ret if np.isfinite(r).any()]
    t = float(np.mean(sds)) if sds else 0.0
    return t if t > 0.0 else 1.0


def _twin(eng, cand, start, value, gamma, H):
    """the yardstick for `cand`: the plain call's (ret, L, fobs), the replayed terminal bits and the bootstrapped twin returns"""
    ret, L, fobs = eng.evaluate_sequences(cand, discount=gamma, start_state=start, final_obs=True)
    ended = _ended(eng, cand, start)
    ret, L = ret.cpu().numpy(), L.cpu().numpy()
    assert ((L < H) <= ended).all()  # the replay's terminal bits cover the short lengths (one at the last step leaves L == H)
    return dict(ret=ret, L=L, fobs=fobs.cpu().numpy(), ended=ended, boot=_bootstrap(ret, ended, fobs, value, gamma, H))


def _members(eng, K):
    """the elite set of the last plan_cem(value=) call: behind the 16-byte records of the workspace, one float64 per candidate, which
    the finish kernel overwrites with the 0 / 1 membership"""
    nk = eng.n_envs * K
    off = 2 * ((nk + 63) // 64 + eng.n_envs)
    return eng._plan_value_ws[off:off + nk].view(eng.n_envs, K).cpu().numpy() != 0


@functools.lru_cache(maxsize=None)
def _run(case, N, K, H, widths, draws, env_kw=()):
    """one start: the candidates written out, the twin, and every output of the four value calls, as NumPy"""
    eng = _engine(case, N, **dict(env_kw))
    value = _value(eng, *widths).bind(eng)
    gamma = CASES[case]["discount"]
    start = _start(eng, case)
    eng.set_state(start)
    nom, sigma = _nominal(eng, H, draws)
    cand = eng.sample_candidates(H, K, SEED, nominal=nom, sigma=sigma)
    tw = _twin(eng, cand, start, value, gamma, H)
    kw = dict(discount=gamma, start_state=start, value=value)
    r = dict(tw, cand=cand.cpu().numpy(), act_dim=eng.act_dim, cheetah=CASES[case]["env"] == "HalfCheetahRunning", range=_range(eng),
             step_tol=_step_tol(eng), nominal=None if nom is None else nom.cpu().numpy())
    r["eval"] = tuple(x.cpu().numpy() for x in eng.evaluate_sequences(cand, final_obs=True, **kw))
    r["shooting"] = tuple(x.cpu().numpy() for x in eng.plan_shooting(H, K, SEED, nominal=nom, sigma=sigma, sequence=True, length=True, **kw))
    r["T"] = _temperature(tw["boot"])
    r["mppi"] = tuple(x.cpu().numpy() for x in eng.plan_mppi(H, K, SEED, r["T"], nominal=nom, sigma=sigma, ess=True, **kw))
    r["M"] = max(1, K // 3)
    if draws == "map":  # plan_cem's own candidates, under a sigma per entry, with a twin of their own
        smap = _sigma_map(eng, nom)
        ccand = eng.sample_candidates(H, K, SEED, nominal=nom, sigma=smap)
        r["cem_twin"] = dict(_twin(eng, ccand, start, value, gamma, H), cand=ccand.cpu().numpy())
        sigma = smap
    else:
        r["cem_twin"] = r
    r["cem"] = tuple(None if x is None else x.cpu().numpy()
                     for x in eng.plan_cem(H, K, r["M"], SEED, nominal=nom, sigma=sigma, elite_return=True, **kw))
    r["members"] = _members(eng, K)
    r["cap_hits"] = eng.solver_cap_hits()
    eng.close()
    return r


def _check_returns(r, got, want, what):
    print(f"{what}: rel err {rel_err(got, want):.3e}, {np.mean(_bits(got) != _bits(want)):.4f} of the values differ in bits")
    if r["cheetah"]:
        assert rel_err(got, want) <= 1e-9, what
    else:
        assert _same(got, want), what


# ------------------------------------------------------------------------------------------------ 1. evaluate_sequences(value=)
@ALL
def test_evaluate_sequences_equals_the_twin(case, N, K, H, widths, draws):
    r = _run(case, N, K, H, widths, draws)
    ret, L, fobs = r["eval"]
    ended = r["ended"]
    assert ret.shape == (N, K) and ret.dtype == np.float64
    print(f"{case} N={N} K={K} H={H} value {widths}: {int(ended.sum())} of {N * K} candidates terminated, "
          f"{int((ended & (r['L'] == H)).sum())} of them only at the last step, {int((ended.any(1) & ~ended.all(1)).sum())} envs hold both kinds")
    _check_returns(r, ret, r["boot"], "returns")
    assert _same(L, r["L"]) and _same(fobs, r["fobs"])  # unchanged by the value
    if not r["cheetah"]:  # a candidate that terminated keeps the plain return's bits, the last step included
        assert np.array_equal(_bits(ret)[ended], _bits(r["ret"])[ended])
    if not ended.all():
        assert (_bits(ret)[~ended] != _bits(r["ret"])[~ended]).any()  # the value reached the others
    if (case, draws) in MIXED and (N, K, H) == (67, 5, 12):  # the preconditions: a case without both kinds cannot pass silently
        assert ended.any() and not ended.all() and (ended & (r["L"] == H)).any()
    if case == "cartpole-balancing" and (N, K, H) == (3, 70, 12):
        assert (ended.any(1) & ~ended.all(1)).all()  # every env mixes
    assert r["cap_hits"] == 0


# ------------------------------------------------------------------------------------------------ 2. plan_shooting(value=)
@ALL
def test_shooting_picks_the_best_bootstrapped_return(case, N, K, H, widths, draws):
    r = _run(case, N, K, H, widths, draws)
    ret, L, _ = r["eval"]  # evaluate_sequences(sample_candidates(...), value=), held to the twin above
    act, bret, idx, seq, ln = r["shooting"]
    rows, cand = np.arange(N), r["cand"]
    assert idx.dtype == np.int32 and bret.dtype == np.float64 and ln.dtype == np.int32 and act.dtype == cand.dtype
    if r["cheetah"]:
        best = ret.max(1)
        assert (np.abs(ret[rows, idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
        assert rel_err(bret, ret[rows, idx]) <= 1e-9
    else:
        assert np.array_equal(idx, SR.best_of(ret).astype(np.int32))
        assert _same(bret, ret[rows, idx])
    assert np.array_equal(ln, L[rows, idx])
    assert _same(act, cand[0, rows, idx]) and _same(seq, cand[:, rows, idx])


# ------------------------------------------------------------------------------------------------ 3. plan_mppi(value=)
@ALL
def test_mppi_equals_its_definition_on_the_bootstrapped_returns(case, N, K, H, widths, draws):
    """tests/test_gpu_mppi.py:_check_definition with the twin's bootstrapped returns in the place of evaluate_sequences'"""
    r = _run(case, N, K, H, widths, draws)
    ret, T = r["boot"], r["T"]
    with np.errstate(all="ignore"):
        want, wret, widx, wess = MR.mppi(r["cand"], ret, T)
    got, bret, idx, ess = r["mppi"]
    _, sret, sidx, _, _ = r["shooting"]
    tail = (r["act_dim"],) if r["act_dim"] > 1 else ()
    assert got.dtype == np.float32 and bret.dtype == np.float64 and idx.dtype == np.int32 and ess.dtype == np.float64
    assert got.shape == (H, N) + tail and bret.shape == (N,) and idx.shape == (N,) and ess.shape == (N,)
    assert np.array_equal(idx, sidx) and _same(bret, sret)  # the winner is plan_shooting(value=)'s, bit for bit
    tol, ess_tol = r["step_tol"], 1e-12
    lo, hi = r["range"]
    if r["cheetah"]:  # tests/test_gpu_mppi.py: the slack the 1e-9 of r_k gives the soft-max mean and ln ESS
        slack = 1e-9 * np.abs(ret).max() / T
        tol, ess_tol = tol + (hi - lo) * slack, ess_tol + 8 * slack
        assert rel_err(bret, wret) <= 1e-9
        best = ret.max(1)
        assert (np.abs(ret[np.arange(N), idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
    else:
        assert np.array_equal(idx, widx) and np.array_equal(bret, wret, equal_nan=True)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    ess_err = np.abs(ess - wess) / wess
    print(f"{case} N={N} K={K} H={H} T={T:.4g}: max |nominal_out - reference| = {err:.3e} (bound {tol:.3e}), ess rel err "
          f"{ess_err.max():.3e} (bound {ess_tol:.1e}), reference ess {wess.min():.3f} .. {wess.max():.3f}")
    assert np.isfinite(got).all() and err <= tol and (ess_err <= ess_tol).all()
    assert got.min() >= lo and got.max() <= hi


# ------------------------------------------------------------------------------------------------ 4. plan_cem(value=)
@ALL
def test_cem_equals_its_definition_on_the_bootstrapped_returns(case, N, K, H, widths, draws):
    """tests/test_gpu_cem.py:_check_definition with the twin's bootstrapped returns in the place of evaluate_sequences'"""
    r = _run(case, N, K, H, widths, draws)
    tw, M = r["cem_twin"], r["M"]
    cand, ret = tw["cand"], tw["boot"]
    lo, hi = r["range"]
    discrete = r["act_dim"] == 0
    with np.errstate(all="ignore"):
        want = CR.cem(cand, ret, M, nominal=r["nominal"], lo=None if discrete else lo, hi=None if discrete else hi)
    mean, std, bret, idx, er = r["cem"]
    members = r["members"]
    assert mean.dtype == np.float32 and bret.dtype == np.float64 and idx.dtype == np.int32 and er.dtype == np.float64
    assert (std is None) == discrete
    if draws != "map":  # the same candidates: the winner is plan_shooting(value=)'s, bit for bit
        assert np.array_equal(idx, r["shooting"][2]) and _same(bret, r["shooting"][1])
    same = lambda a, b: np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))
    if r["cheetah"]:
        srt = -np.sort(-ret, axis=1)
        if M < K:
            gap = srt[:, M - 1] - srt[:, M]
            assert (gap > 1e-6 * np.maximum(np.abs(srt[:, M - 1]), 1e-3)).all(), "precondition: choose another seed"
        assert rel_err(bret, want.best_return) <= 1e-9 and rel_err(er, want.elite_return) <= 1e-9
        best = ret.max(1)
        assert (np.abs(ret[np.arange(N), idx] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
    else:
        assert np.array_equal(idx, want.best_index) and same(bret, want.best_return) and same(er, want.elite_return)
    assert (members.sum(1) == M).all() and np.array_equal(members, want.members)
    tol = r["step_tol"]
    err = np.abs(mean.astype(np.float64) - want.mean.astype(np.float64)).max()
    print(f"{case} N={N} K={K} M={M} H={H}: max |mean_out - reference| = {err:.3e} (bound {tol:.3e})")
    assert np.isfinite(mean).all() and err <= tol
    if std is not None:
        sbound = float(np.spacing(np.float32(hi - lo))) + K * 2.0 ** -52 * want.s2_over_m / np.maximum(want.std64, TINY)
        serr = np.abs(std.astype(np.float64) - want.std.astype(np.float64))
        print(f"    max |std_out - reference| = {serr.max():.3e} (bound {sbound.min():.3e} .. {sbound.max():.3e})")
        assert np.isfinite(std).all() and (std >= 0).all() and (serr <= sbound).all()
    plo, phi = (0.0, 1.0) if discrete else (lo, hi)
    assert mean.min() >= plo and mean.max() <= phi


# ------------------------------------------------------------------------------------------------ 5. at the cap: the 64 KiB tile
@pytest.mark.parametrize("case", ["cartpole-balancing", "cheetah"])
def test_widths_256(case):
    """the launches that need the opt-in for 64 KiB of dynamic LDS on the new kernels, next to the cheetah's static LDS"""
    N, K, H = 3, 5, 1
    r = _run(case, N, K, H, (256, 256), None)
    _check_returns(r, r["eval"][0], r["boot"], f"{case} 256x256 returns")
    assert _same(r["eval"][1], r["L"]) and _same(r["eval"][2], r["fobs"])
    rows = np.arange(N)
    act, bret, idx, seq, ln = r["shooting"]
    _check_returns(r, bret, r["eval"][0][rows, idx], "best_return")
    assert _same(act, r["cand"][0, rows, idx]) and np.array_equal(ln, r["L"][rows, idx])
    for wret, widx in (r["mppi"][1:3], r["cem"][2:4]):  # the three planners agree on the winner
        assert _same(wret, bret) and np.array_equal(widx, idx)
    if not r["ended"].all():
        assert (_bits(r["eval"][0])[~r["ended"]] != _bits(r["ret"])[~r["ended"]]).any()
    assert r["cap_hits"] == 0


# ------------------------------------------------------------------------------------------------ 6. the action dtypes
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_given_candidates_in_every_action_dtype(dtype):
    case, N, K, H = "cartpole-balancing", 67, 5, 12
    r = _run(case, N, K, H, (3, 4), None)
    eng = _engine(case, N)
    value = _value(eng, 3, 4)
    cand = torch.as_tensor(r["cand"], device=eng.device).to(getattr(torch, dtype)).contiguous()
    ret, L, fobs = eng.evaluate_sequences(cand, discount=CASES[case]["discount"], start_state=_start(eng, case), final_obs=True, value=value)
    assert _same(ret.cpu().numpy(), r["boot"]) and _same(L.cpu().numpy(), r["L"]) and _same(fobs.cpu().numpy(), r["fobs"])
    ret2, L2 = eng.evaluate_sequences(cand, discount=CASES[case]["discount"], start_state=_start(eng, case), value=value)  # no final_obs
    assert torch.equal(ret2, ret) and torch.equal(L2, L)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. direction
def _constant_critic(eng, b3):
    from emei_amd.policy import DeepValueFunction

    z = lambda *s: torch.zeros(s)
    return DeepValueFunction(z(1, 2), torch.full((1,), float(b3)), z(2, 3), z(2), z(3, eng.obs_dim), z(3))


def test_a_constant_critic_moves_the_winner_the_way_its_sign_says():
    """CartPoleBalancing pays 1 per step: with V = +100 everywhere a never-terminated candidate wins wherever there is one, with
    V = -100 a terminated one does, and with V = 0 every output equals the plain call's"""
    case, N, K, H = "cartpole-balancing", 67, 5, 12
    r = _run(case, N, K, H, (3, 4), None)
    ended = r["ended"]
    both = ended.any(1) & ~ended.all(1)
    assert both.sum() >= 10
    eng = _engine(case, N)
    start = _start(eng, case)
    cand = torch.as_tensor(r["cand"], device=eng.device)
    rows = np.arange(N)
    for b3, want_ended in ((100.0, False), (-100.0, True)):
        v = _constant_critic(eng, b3)
        picks = [eng.plan_shooting(H, K, SEED, start_state=start, value=v)[2], eng.plan_mppi(H, K, SEED, 1.0, start_state=start, value=v)[2],
                 eng.plan_cem(H, K, 2, SEED, start_state=start, value=v)[3]]
        for idx in picks:
            idx = idx.cpu().numpy()
            assert (ended[rows, idx][both] == want_ended).all(), b3
        ret = eng.evaluate_sequences(cand, start_state=start, value=v)[0].cpu().numpy()
        assert _same(ret, np.where(ended, r["ret"], r["ret"] + b3))  # discount 1: g_H = 1
    zero = _constant_critic(eng, 0.0)
    calls = (lambda **kw: eng.evaluate_sequences(cand, start_state=start, final_obs=True, **kw),
             lambda **kw: eng.plan_shooting(H, K, SEED, start_state=start, sequence=True, length=True, **kw),
             lambda **kw: eng.plan_mppi(H, K, SEED, 0.7, start_state=start, ess=True, **kw),
             lambda **kw: eng.plan_cem(H, K, 2, SEED, start_state=start, elite_return=True, **kw))
    for call in calls:
        for x, y in zip(call(value=zero), call()):
            assert (x is None and y is None) or torch.equal(x, y)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. iterations
def test_cem_iterations_use_the_value_in_every_iteration():
    import emei_amd

    N, K, M, H = 5, 13, 4, 5
    env = emei_amd.make("HopperRunning-v0", num_envs=N)
    env.reset(seed=7)
    eng = env.engine
    value = _value(eng, 9, 2)
    got = env.plan_cem(H, K, M, 50, discount=0.97, iterations=2, elite_return=True, value=value)
    first = eng.plan_cem(H, K, M, 50, discount=0.97, value=value)
    nom, sig = first[0].clone(), first[1].clone()
    want = eng.plan_cem(H, K, M, 51, discount=0.97, nominal=nom, sigma=sig, elite_return=True, value=value)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    plain = eng.plan_cem(H, K, M, 51, discount=0.97, nominal=nom, sigma=sig, elite_return=True)
    assert not torch.equal(plain[2], want[2])  # the second iteration's returns carry the value
    assert eng.solver_cap_hits() == 0


# ------------------------------------------------------------------------------------------------ 9. the contract
def _outputs(eng, H, K, value, nominal=None, sigma=None, **kw):
    """every output of the three planners and of evaluate_sequences on the candidates they draw"""
    cand = eng.sample_candidates(H, K, SEED, nominal=nominal, sigma=sigma)
    kw = dict(kw, value=value)
    return (eng.evaluate_sequences(cand, final_obs=True, **kw)
            + eng.plan_shooting(H, K, SEED, nominal=nominal, sigma=sigma, sequence=True, length=True, **kw)
            + eng.plan_mppi(H, K, SEED, 0.6, nominal=nominal, sigma=sigma, ess=True, **kw)
            + eng.plan_cem(H, K, 2, SEED, nominal=nominal, sigma=sigma, elite_return=True, **kw))


def test_handle_untouched():
    case, N = "hopper-terminating", 96
    a, b = _engine(case, N, max_episode_steps=9), _engine(case, N, max_episode_steps=9)
    g = torch.Generator(device=a.device).manual_seed(9)
    step_acts = torch.rand((20, N, a.act_dim), generator=g, device=a.device) * 2 - 1
    for e in (a, b):
        e.rollout(step_acts[:7], auto_reset=True)
        e.freeze()
        e.rollout(step_acts[7:12], auto_reset=True)
    kernel = a.last_kernel()
    _outputs(a, 12, 5, _value(a, 9, 2), discount=0.9)
    assert a.last_kernel() == kernel == b.last_kernel()
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.compact_done(), b.compact_done())
    for x, y in zip(a.get_counters(), b.get_counters()):
        assert torch.equal(x, y)
    outs = [e.rollout(step_acts, auto_reset=True) for e in (a, b)]  # auto-reset: the reset key is the handle's own still
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    for e in (a, b):
        e.unfreeze()  # the snapshot is the one freeze() took
    assert torch.equal(a.get_state(), b.get_state())
    for e in (a, b):
        e.close()


def test_start_state_argument_equals_set_state():
    case = "cartpole-balancing"
    eng = _engine(case, 67)
    value = _value(eng, 9, 2)
    start = _start(eng, case) + 0.01
    want = _outputs(eng, 12, 5, value, discount=0.99, start_state=start)
    assert torch.equal(eng.get_state(), _engine(case, 67).get_state())  # the handle's own state is not the start
    eng.set_state(start)
    got = _outputs(eng, 12, 5, value, discount=0.99)
    for x, y in zip(got, want):
        assert (x is None and y is None) or torch.equal(x, y)
    eng.close()


def test_shards_give_the_whole():
    case, N, K, H = "hopper-terminating", 134, 5, 12
    whole = _engine(case, N)
    start = _start(whole, case)
    nom = torch.zeros((H, N, whole.act_dim), dtype=torch.float32, device=whole.device)
    want = _outputs(whole, H, K, _value(whole, 9, 2), nominal=nom, sigma=0.5, discount=0.97, start_state=start)
    got = []
    for o, n in ((0, 67), (67, 67)):
        part = _engine(case, n, env_index_offset=OFFSET + o)
        got.append(_outputs(part, H, K, _value(part, 9, 2), nominal=nom[:, o:o + n].contiguous(), sigma=0.5, discount=0.97,
                            start_state=start[o:o + n].contiguous()))
        part.close()
    for q, w in enumerate(want):
        dim = 1 if w.dim() >= 2 and w.shape[0] == H and w.shape[1] == N else 0  # [H, N, ..] outputs are cut along the envs
        assert torch.equal(torch.cat([g[q] for g in got], dim=dim), w), q
    assert not torch.equal(want[0][:67], want[0][67:])  # the shards do not simply repeat each other
    whole.close()


def _raw(eng, which, H, K, value, skip=None):
    """the ABI call `which` with every optional output, or with `skip` NULL -> {name: tensor}"""
    from emei_amd import _lib as L
    from emei_amd.engine import _ACT_DTYPES, _ptr, _stream

    N = eng.n_envs
    vs = value.bind(eng).struct()
    dtype = torch.int64 if eng.act_dim == 0 else torch.float32
    new = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=eng.device)
    tail = eng._act_tail
    ws = torch.empty(L.lib().emei_plan_value_workspace_bytes(N, K) // 8, dtype=torch.float64, device=eng.device)
    f64, i32 = torch.float64, torch.int32
    if which == "evaluate":
        cand = eng.sample_candidates(H, K, SEED)
        out = dict(ret=new((N, K), f64), len=new((N, K), i32), fobs=new((N, K, eng.obs_dim), torch.float32))
        p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
        call = lambda: L.lib().emei_evaluate_sequences_value(eng._h, H, K, _ptr(cand), _ACT_DTYPES[cand.dtype], 0.97, C.byref(vs), None,
                                                             p["ret"], p["len"], p["fobs"], _stream())
    elif which == "shooting":
        out = dict(act=new((N,) + tail, dtype), seq=new((H, N) + tail, dtype), ret=new((N,), f64), idx=new((N,), i32), len=new((N,), i32))
        p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
        call = lambda: L.lib().emei_plan_shooting_value(eng._h, H, K, SEED, None, 0.0, 0.97, C.byref(vs), None, _ptr(ws), p["act"],
                                                        _ACT_DTYPES[dtype], p["seq"], p["ret"], p["idx"], p["len"], _stream())
    elif which == "mppi":
        out = dict(nom=new((H, N) + tail, torch.float32), ret=new((N,), f64), idx=new((N,), i32), ess=new((N,), f64))
        p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
        call = lambda: L.lib().emei_plan_mppi_value(eng._h, H, K, SEED, None, 0.0, 0.97, C.byref(vs), 0.5, None, _ptr(ws), p["nom"],
                                                    p["ret"], p["idx"], p["ess"], _stream())
    else:
        out = dict(mean=new((H, N) + tail, torch.float32), ret=new((N,), f64), idx=new((N,), i32), er=new((N,), f64))
        if eng.act_dim > 0:
            out["std"] = new((H, N) + tail, torch.float32)
        p = {k: (None if k == skip else _ptr(v)) for k, v in out.items()}
        call = lambda: L.lib().emei_plan_cem_value(eng._h, H, K, 2, SEED, None, 0.0, None, 0.97, C.byref(vs), None, _ptr(ws), p["mean"],
                                                   p.get("std"), p["ret"], p["idx"], p["er"], _stream())
    with torch.cuda.device(eng.device):
        L.check(call())
    torch.cuda.synchronize()
    return out


OPTIONAL = {"evaluate": ("fobs",), "shooting": ("seq", "len"), "mppi": ("ret", "idx", "ess"), "cem": ("std", "ret", "idx", "er")}


@pytest.mark.parametrize("which", sorted(OPTIONAL))
def test_null_outputs_one_at_a_time(which):
    case = "hopper-terminating"
    eng = _engine(case, 67)
    eng.set_state(_start(eng, case))
    value = _value(eng, 9, 2)
    full = _raw(eng, which, 12, 5, value)
    assert all(not (v == 77).all() for v in full.values())
    for skip in OPTIONAL[which]:
        got = _raw(eng, which, 12, 5, value, skip=skip)
        for k, v in got.items():
            if k == skip:
                assert (v == 77).all(), k  # not written
            else:
                assert torch.equal(v, full[k]), (skip, k)
    eng.close()


def test_capture_replays_the_same_result():
    N, K, H = 67, 5, 12
    case = "hopper-terminating"
    eng = _engine(case, N)
    eng.set_state(_start(eng, case))
    value = _value(eng, 9, 2).bind(eng)
    want = _outputs(eng, H, K, value, discount=0.99)
    cand = eng.sample_candidates(H, K, SEED)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    kw = dict(discount=0.99, value=value)
    with torch.cuda.graph(graph, stream=side):  # one linear chain: the four calls' seven launches
        got = (eng.evaluate_sequences(cand, final_obs=True, **kw) + eng.plan_shooting(H, K, SEED, sequence=True, length=True, **kw)
               + eng.plan_mppi(H, K, SEED, 0.6, ess=True, **kw) + eng.plan_cem(H, K, 2, SEED, elite_return=True, **kw))
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for x in got:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    eng.close()


# ------------------------------------------------------------------------------------------------ 10. refusals that need a handle
def test_refusals_on_a_handle():
    from emei_amd import _lib as L
    from emei_amd.engine import Engine, _ptr, _stream
    from test_gpu_policy_plan_deep import BODY

    eng = Engine("HopperRunning", 4, **BODY)
    value = _value(eng, 9, 2)
    for call in (lambda **kw: eng.plan_shooting(3, 2, 0, value=value, **kw), lambda **kw: eng.plan_mppi(3, 2, 0, 1.0, value=value, **kw),
                 lambda **kw: eng.plan_cem(3, 2, 1, 0, value=value, **kw)):
        with pytest.raises(AssertionError):  # EMEI_ERR_STATE: no reset yet and no start_state
            call()
        out = call(start_state=torch.zeros((4, eng.state_dim), dtype=torch.float64, device=eng.device))
        assert out[0].shape[-1] == 3  # a start_state stands in for the state
    eng.reset(seed=0)
    vs = value.bind(eng).struct()
    N, K = 4, 2
    ws = torch.empty(L.lib().emei_plan_value_workspace_bytes(N, K) // 8, dtype=torch.float64, device=eng.device)
    buf = {k: torch.zeros(64, dtype=torch.float64, device=eng.device) for k in ("a", "b", "c", "d", "nom", "smap")}
    p = {k: _ptr(v) for k, v in buf.items()}
    lib = L.lib()

    def weights(null):
        s = value.struct()
        setattr(s, null, None)
        return s

    def shooting(vs=vs, K=K, dtype=L.ACT_F32, work=_ptr(ws), act=p["a"], nominal=None, sigma=0.0):
        with torch.cuda.device(eng.device):
            rc = lib.emei_plan_shooting_value(eng._h, 3, K, 7, nominal, sigma, 1.0, C.byref(vs), None, work, act, dtype, None, p["b"], p["c"],
                                              None, _stream())
        return rc, lib.emei_last_error().decode()

    FN = "emei_plan_shooting_value:"
    # the value's weights come first behind the handle, in the header's order, then the plain call's remaining checks in its order
    for name in ("w1", "b1", "w2", "b2", "w3", "b3"):
        rc, msg = shooting(vs=weights(name), K=2 ** 30, dtype=L.ACT_U8, work=None)
        assert rc == L.ERR_INVALID and msg.startswith(FN) and f"null value.{name}" in msg, msg
    s = value.struct()
    s.w2 = s.b3 = None
    assert "null value.w2" in shooting(vs=s)[1]
    for kw, word in ((dict(nominal=p["nom"], sigma=-1.0), "sigma"), (dict(K=2 ** 30), "n_envs * n_candidates")):
        rc, msg = shooting(dtype=L.ACT_U8, work=None, **kw)
        assert rc == L.ERR_INVALID and msg.startswith(FN) and word in msg, (kw, msg)
    assert shooting(dtype=L.ACT_U8, work=None)[0] == L.ERR_INVALID  # a wrong action_dtype, before the pointers
    rc, msg = shooting(work=None)
    assert rc == L.ERR_INVALID and msg.startswith(FN) and "null argument" in msg, msg
    assert shooting(act=None)[0] == L.ERR_INVALID
    assert shooting()[0] == L.OK

    def mppi(work=_ptr(ws), out=p["a"], vs=vs):
        with torch.cuda.device(eng.device):
            rc = lib.emei_plan_mppi_value(eng._h, 3, K, 7, None, 0.0, 1.0, C.byref(vs), 1.0, None, work, out, None, None, None, _stream())
        return rc, lib.emei_last_error().decode()

    assert "null value.b2" in mppi(vs=weights("b2"), work=None)[1]
    for kw, word in ((dict(work=None), "workspace"), (dict(out=None), "nominal_out")):
        rc, msg = mppi(**kw)
        assert rc == L.ERR_INVALID and msg.startswith("emei_plan_mppi_value:") and word in msg, (kw, msg)
    assert mppi()[0] == L.OK

    def cem(h=None, work=_ptr(ws), mean=p["a"], std=None, nominal=None, smap=None, vs=vs):
        h = eng._h if h is None else h
        with torch.cuda.device(eng.device):
            rc = lib.emei_plan_cem_value(h, 3, K, 1, 7, nominal, 0.1, smap, 1.0, C.byref(vs), None, work, mean, std, None, None, None, _stream())
        return rc, lib.emei_last_error().decode()

    assert "null value.w3" in cem(vs=weights("w3"), smap=p["smap"])[1]
    for kw, word in ((dict(smap=p["smap"]), "sigma_map"), (dict(work=None), "workspace"), (dict(mean=None), "mean_out")):
        rc, msg = cem(**kw)
        assert rc == L.ERR_INVALID and msg.startswith("emei_plan_cem_value:") and word in msg, (kw, msg)
    assert cem(nominal=p["nom"], smap=p["smap"], std=p["b"])[0] == L.OK
    cart = Engine("CartPoleSwingUp", 4)
    cart.reset(seed=0)
    cvs = _value(cart, 3, 4).bind(cart).struct()
    for kw in (dict(nominal=p["nom"], smap=p["smap"]), dict(std=p["b"])):
        rc, msg = cem(h=cart._h, vs=cvs, **kw)
        assert rc == L.ERR_INVALID and "discrete" in msg, (kw, msg)
    # evaluate_sequences_value: the pointers, then a dtype the env does not take
    acts = torch.zeros((3, N, K, 3), device=eng.device)

    def evaluate(actions=_ptr(acts), ret=p["a"], ln=p["b"], dtype=L.ACT_F32, vs=vs):
        with torch.cuda.device(eng.device):
            rc = lib.emei_evaluate_sequences_value(eng._h, 3, K, actions, dtype, 1.0, C.byref(vs), None, ret, ln, None, _stream())
        return rc, lib.emei_last_error().decode()

    assert "null value.b1" in evaluate(vs=weights("b1"), actions=None)[1]
    for kw in (dict(actions=None), dict(ret=None), dict(ln=None)):
        rc, msg = evaluate(**kw)
        assert rc == L.ERR_INVALID and msg.startswith("emei_evaluate_sequences_value:") and "null argument" in msg, (kw, msg)
    assert evaluate(dtype=L.ACT_I64)[0] == L.ERR_INVALID and evaluate()[0] == L.OK
    with pytest.raises(ValueError, match="obs_dim"):
        cart.plan_mppi(3, 2, 0, 1.0, value=value)  # a value of another env's shape
    with pytest.raises(TypeError, match="DeepValueFunction"):
        eng.plan_mppi(3, 2, 0, 1.0, value=lambda o: o)
    torch.cuda.synchronize()
    eng.close()
    cart.close()
