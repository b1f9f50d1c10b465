"""tests/policy_population_reference.py:evaluate_policies, the numpy twin of emei_evaluate_policies, held on the CPU against the
references the project already has, on a population of one: its actions are policy_reference.mlp_actions of the rows the text says
the policy sees, its per-step outputs are plan_reference.oracle_steps of those actions, and its (return, length, final observation)
are plan_reference.contract of those outputs — all exactly.  (contract sums with math.fsum; the twin's running float64 sum of at
most 40 widened float32 rewards of one magnitude rounds nowhere, so at discount 1 the two agree to the bit; under a discount the
twin is held, exactly, to the text's running product and sum written out once more, and to contract within float64 rounding.)
Then: members of a population do not see one another, and the inputs tests/test_gpu_policy_population.py uses exercise the early exit
— lengths below the horizon and lengths equal to it, returns that tell the members apart — as the CPU oracle steps them."""
import numpy as np
import pytest

import plan_reference as R
import policy_population_reference as PP
import policy_reference as PR

ONE = [("CartPoleBalancing", {}, 40, 0), ("CartPoleBalancing", {}, 40, 5), ("ReboundInvertedPendulumBalancing", {}, 12, 0),
       ("ReboundInvertedPendulumBalancing", {}, 33, 5)]


def _inputs(name, hidden, N=37):
    fam = R.FAMILY[name][0]
    s0, _ = R.BUILDERS[fam](name, N, 1, 1, 900 + hidden)
    pol = PP.cartpole_balancing_population(hidden)[1] if fam == "cartpole" else PP.random_population(4, 1, hidden, 1, 901)[0]
    return s0, pol


@pytest.mark.parametrize("name,kw,H,hidden", ONE)
@pytest.mark.parametrize("discount", [1.0, 0.95])
def test_a_population_of_one_against_the_policy_and_plan_references(name, kw, H, hidden, discount):
    s0, pol = _inputs(name, hidden)
    got = PP.evaluate_policies(name, kw, s0, [pol], H, discount)
    assert got["ret"].shape == got["L"].shape == (1, len(s0)) and got["final_obs"].shape == (1, len(s0), 4)
    acts, obs, rew, term = got["actions"][0], got["obs"][0], got["reward"][0], got["terminal"][0]
    # the policy reference on the rows the text names: x_0 from the start state, then every emitted row, rounded to float32
    seen = np.concatenate([PP.first_observation(name, s0)[None], obs[:-1]]).astype(np.float32)
    lo, hi = PR.ctrl_range(name)
    for t in range(H):
        want = PR.mlp_actions(pol, seen[t], lo, hi, R.FAMILY[name][0] == "cartpole")
        assert np.array_equal(np.asarray(want).reshape(-1), np.asarray(acts[t]).reshape(-1)), t
    # the plan reference on those actions, open loop
    o2, r2, d2 = R.oracle_steps(name, kw, s0, acts)
    assert np.array_equal(o2, obs) and np.array_equal(r2, rew) and r2.dtype == np.float32 and np.array_equal(d2, term)
    ret, L, fo = R.contract(o2, r2, d2, discount)
    assert np.array_equal(got["L"][0], L) and got["L"].dtype == np.int32 and np.array_equal(got["final_obs"][0], fo)
    if discount == 1.0:
        assert np.array_equal(got["ret"][0], ret)
    else:
        text = np.zeros(len(s0))
        for m in range(len(s0)):
            g = 1.0
            for t in range(L[m]):
                text[m] = text[m] + g * float(np.float64(r2[t, m]))
                g = g * discount
        assert np.array_equal(got["ret"][0], text)
        assert np.abs(got["ret"][0] - ret).max() <= 2 * H * np.finfo(np.float64).eps * np.abs(r2).sum(axis=0).max()
    if name == "CartPoleBalancing":  # both kinds of pair are covered
        assert (L < H).any() and (L == H).any()


def test_members_do_not_see_one_another():
    s0, _ = R.cartpole_inputs("CartPoleBalancing", 37, 1, 1, 77)
    pop = PP.cartpole_balancing_population(5)
    whole = PP.evaluate_policies("CartPoleBalancing", {}, s0, pop, 40, 0.97)
    for p, member in enumerate(pop):
        alone = PP.evaluate_policies("CartPoleBalancing", {}, s0, [member], 40, 0.97)
        for k in whole:
            assert np.array_equal(whole[k][p], alone[k][0]), (p, k)


@pytest.mark.parametrize("hidden", [0, 5])
def test_the_gpu_inputs_exercise_the_early_exit(hidden):
    """what tests/test_gpu_policy_population.py asserts on the device's reference route, shown first on the CPU oracle"""
    s0 = PP.gpu_start("CartPoleBalancing", 130)
    cp = PP.evaluate_policies("CartPoleBalancing", {}, s0, PP.cartpole_balancing_population(hidden), 40, 1.0)
    s0 = PP.gpu_start("HopperRunning", 70)
    hop = PP.evaluate_policies("HopperRunning", PP.HOPPER_TERMINATING, s0, PP.hopper_population(hidden), 12, 1.0)
    for r, H in ((cp, 40), (hop, 12)):
        assert (r["L"] < H).any() and (r["L"] == H).any()
        P = len(r["ret"])
        assert all(not np.array_equal(r["ret"][p], r["ret"][q]) for p in range(P) for q in range(p))
    # with the Hopper's default parameters no step is ever terminal (hopper.py:104-106), whatever the policy does
    dflt = PP.evaluate_policies("HopperRunning", dict(R.MUJOCO, integrator="rk4"), s0, PP.hopper_population(hidden), 12, 1.0)
    assert (dflt["L"] == 12).all() and not dflt["terminal"].any()
