"""tests/plan_reference.py on the CPU: (a) `contract` against a scalar Python loop on a hand-made case; (b) every case of
tests/test_gpu_plan_oracle.py meets its input conditions from the oracle alone — the lengths that must occur do occur and
almost no candidate sits on a terminal threshold — before any GPU is involved."""
import numpy as np
import pytest

import plan_reference as P


def _scalar_loop(obs, rew, term, discount):
    """one candidate, the header text word for word"""
    H = len(rew)
    L = H
    for t in range(H):
        if term[t]:
            L = t + 1
            break
    ret = 0.0
    for t in range(L):
        ret += discount**t * float(np.float32(rew[t]))
    return ret, L, obs[L - 1]


@pytest.mark.parametrize("discount", [1.0, 0.9])
def test_contract_equals_a_scalar_loop(discount):
    H = 6
    # columns: terminal at step 0; at the last step; two terminals (steps 2 and 4: only the first counts); none at all
    term = np.zeros((H, 4), bool)
    term[0, 0] = term[H - 1, 1] = term[2, 2] = term[4, 2] = True
    rng = np.random.default_rng(0)
    rew = rng.uniform(-2, 2, (H, 4)).astype(np.float32)
    obs = rng.normal(size=(H, 4, 3))
    ret, L, fo = P.contract(obs, rew, term, discount)
    assert L.dtype == np.int32 and L.tolist() == [1, H, 3, H]
    for m in range(4):
        w_ret, w_L, w_fo = _scalar_loop(obs[:, m], rew[:, m], term[:, m], discount)
        assert L[m] == w_L and np.array_equal(fo[m], w_fo)
        assert abs(ret[m] - w_ret) <= 4 * np.finfo(np.float64).eps * np.abs(rew[:w_L, m]).sum()  # fsum against a running sum
    assert ret[0] == float(rew[0, 0])  # discount^0 = 1: the terminal step's own reward, nothing after it
    # the steps after the first terminal do not count: changing them changes nothing
    rew2, obs2 = rew.copy(), obs.copy()
    rew2[3:, 2], obs2[3:, 2] = 7.0, 9.0
    ret2, L2, fo2 = P.contract(obs2, rew2, term, discount)
    assert np.array_equal(ret2, ret) and np.array_equal(L2, L) and np.array_equal(fo2, fo)
    b = P.ret_bound(rew, L, discount, 1e-5)
    assert b[0] == pytest.approx(1e-5 * max(abs(float(rew[0, 0])), 1e-3))


def test_undecidable_marks_rows_on_a_threshold_only():
    """CartPoleBalancing ends at |x| >= 2.4 (cartpole.py): a row 1e-6 relative inside the threshold flips under the 1e-5 move, a
    row 1e-3 inside does not, and a flip after the candidate's last counted step does not count."""
    obs = np.zeros((2, 3, 4))
    obs[0, 0, 0] = 2.4 * (1 - 1e-6)
    obs[0, 1, 0] = -2.4 * (1 - 1e-3)
    obs[1, 2, 0] = 2.4 * (1 + 1e-6)
    assert P.undecidable("CartPoleBalancing", obs, np.array([2, 2, 2])).tolist() == [True, False, True]
    assert P.undecidable("CartPoleBalancing", obs, np.array([2, 2, 1])).tolist() == [True, False, False]


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_case_inputs_meet_their_conditions(case):
    assert (case.N * case.K) % 64 and case.N % 64 and 64 % case.K and case.N * case.K > 64  # ragged block, straddled waves
    a, b = case.build(), case.build()
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].dtype == np.float64  # the GPU test sees the same inputs
    ref = P.reference(case)
    L, H = ref["L"], case.H
    assert np.isfinite(ref["obs"]).all() and np.isfinite(ref["reward"]).all()
    assert ref["skip"].mean() <= 0.01, ref["skip"].mean()
    if case.ends:
        early, full, distinct = float((L < H).mean()), float((L == H).mean()), len(np.unique(L))
        assert early >= 0.30 and full >= 0.05 and distinct >= 8, (early, full, distinct)
    else:
        assert L.max() == H
    assert (ref["bound"] > 0).all()


def _mutants(case, ref):
    """the planner's likely mistakes applied to the oracle's per-step outputs: {name: (ret, L, final_obs)}"""
    obs, rew, term, g = ref["obs"], ref["reward"], ref["terminal"], case.discount
    H, M = rew.shape
    ret, L, fo = ref["ret"], ref["L"], ref["final_obs"]
    r64, cols = rew.astype(np.float64), np.arange(M)
    ended = term[L - 1, cols]  # the candidate's last counted step is a terminal one
    out = {"reward added after the live update": (ret - np.where(ended, g ** (L - 1) * r64[L - 1, cols], 0.0), L, fo),
           "len = t": (ret, np.where(ended, L - 1, L), fo),
           "final_obs of step L": (ret, L, obs[np.minimum(L, H - 1), cols])}
    if g < 1.0:
        out["g advanced before use"] = (ret * g, L, fo)
    # i = j % K: candidate j starts from row (j % K) % N and not from row j // K (the actions stay where they are)
    s0, acts = case.build()
    rows = s0[(cols % case.K) % case.N]
    o2, r2, t2 = P.oracle_steps(case.name, case.kw, rows, acts.reshape((H, M) + acts.shape[3:]))
    out["i = j % K"] = P.contract(o2, r2, t2, g)
    # the action prefetch clamped to step H - 2: the last step repeats the action before it
    a2 = acts.reshape((H, M) + acts.shape[3:]).copy()
    a2[H - 1] = a2[H - 2]
    out["prefetch clamped to last - 1"] = P.contract(*P.oracle_steps(case.name, case.kw, np.repeat(s0, case.K, axis=0), a2), g)
    return out


@pytest.mark.parametrize("case", [c for c in P.CASES if c.ends], ids=[c.tag for c in P.CASES if c.ends])
def test_the_bounds_tell_a_wrong_contract_from_the_right_one(case):
    """The reference compared with itself passes, and each mistake a plan kernel could make — applied here to the oracle's own
    per-step outputs — breaks at least one of the three assertions of tests/test_gpu_plan_oracle.py on this case's inputs."""
    ref = P.reference(case)
    wrong, r_ratio, o_ratio = P.compare(case, ref, ref["ret"], ref["L"], ref["final_obs"])
    assert wrong.size == 0 and r_ratio == 0.0 and o_ratio == 0.0
    for name, (ret, L, fo) in _mutants(case, ref).items():
        wrong, r_ratio, o_ratio = P.compare(case, ref, ret, L, fo)
        assert wrong.size > 0 or r_ratio > 1.0 or o_ratio > 1.0, name
