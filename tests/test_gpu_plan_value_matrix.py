"""The four value calls (evaluate_sequences / plan_shooting / plan_mppi / plan_cem with value=) on every compiled kernel
configuration: the 64 rows of tests/kernel_matrix.py, each a translation unit of the Makefile and an integrator, which is what
instantiates pend_plan_value_kernel / body_plan_value_kernel.  One small shape per row — N = 3, K = 70 (an env over two waves, a
ragged last wave), H = 2, value widths (5, 3) (a ragged group of h1, h2 below the second layer's block) — from Row.states, the start
rows that activate the family's constraints.  The returns are held to the twin of tests/test_gpu_plan_value.py: the plain
evaluate_sequences, the terminal bits of the replayed rollouts and DeepValueFunction.__call__ — bit for bit, 1e-9 relative on the
HalfCheetah rows; the planners' winners, means and elite sets to shooting_reference / mppi_reference / cem_reference on those returns."""
import numpy as np
import pytest

import cem_reference as CR
import kernel_matrix as KM
import mppi_reference as MR
import shooting_reference as SR
from conftest import rel_err
from test_gpu_kernel_matrix import _engine
from test_gpu_plan_value import _members, _range, _step_tol, _twin
from test_gpu_policy_plan_deep import _same, _value

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, K, H, M = 3, 70, 2, 9
WIDTHS = (5, 3)
GAMMA = 0.97
SEED = 2 ** 33 + 5


@pytest.mark.parametrize("row", KM.ROWS, ids=lambda r: r.id)
def test_value_calls_equal_the_twin(row):
    eng = _engine(row, N)
    cheetah = row.family == "cheetah"
    value = _value(eng, *WIDTHS).bind(eng)
    start = torch.as_tensor(row.states(N), device=eng.device, dtype=torch.float64).contiguous()
    cand = eng.sample_candidates(H, K, SEED)
    tw = _twin(eng, cand, start, value, GAMMA, H)
    boot, ended = tw["boot"], tw["ended"]
    kw = dict(discount=GAMMA, start_state=start, value=value)
    ret, L, fobs = (x.cpu().numpy() for x in eng.evaluate_sequences(cand, final_obs=True, **kw))
    act, bret, idx, ln = (x.cpu().numpy() for x in eng.plan_shooting(H, K, SEED, length=True, **kw))
    T = float(np.std(boot[np.isfinite(boot)])) or 1.0
    nom, mret, midx, ess = (x.cpu().numpy() for x in eng.plan_mppi(H, K, SEED, T, ess=True, **kw))
    cem = eng.plan_cem(H, K, M, SEED, elite_return=True, **kw)
    members = _members(eng, K)
    cmean, cret, cidx, cer = (cem[q].cpu().numpy() for q in (0, 2, 3, 4))
    cand = cand.cpu().numpy()
    rows = np.arange(N)
    print(f"{row.id}: {int(ended.sum())} of {N * K} candidates terminated, returns rel err {rel_err(ret, boot):.3e}")
    assert np.isfinite(boot).all()
    assert _same(L, tw["L"]) and _same(fobs, tw["fobs"])
    if not ended.all():
        assert (ret[~ended] != tw["ret"][~ended]).any()  # the value reached the candidates that never terminated
    lo, hi = _range(eng)
    tol, ess_tol = _step_tol(eng), 1e-12
    with np.errstate(all="ignore"):
        want, wret, widx, wess = MR.mppi(cand, boot, T)
        cwant = CR.cem(cand, boot, M, nominal=None, lo=None if eng.act_dim == 0 else lo, hi=None if eng.act_dim == 0 else hi)
    if cheetah:  # a lane depends on its wave-mates at the 1e-9 level (the constraint-slot lending)
        assert rel_err(ret, boot) <= 1e-9
        best = boot.max(1)
        for r_, i_ in ((bret, idx), (mret, midx), (cret, cidx)):
            assert rel_err(r_, boot[rows, i_]) <= 1e-9 and (np.abs(boot[rows, i_] - best) <= 1e-9 * np.maximum(np.abs(best), 1e-3)).all()
        slack = 1e-9 * np.abs(boot).max() / T
        tol, ess_tol = tol + (hi - lo) * slack, ess_tol + 8 * slack
    else:
        assert _same(ret, boot)
        assert np.array_equal(ret[ended].view(np.uint64), tw["ret"][ended].view(np.uint64))  # a terminated candidate gets nothing
        assert np.array_equal(idx, SR.best_of(boot).astype(np.int32)) and _same(bret, boot[rows, idx])
        assert np.array_equal(midx, widx) and np.array_equal(cidx, cwant.best_index)
        assert np.array_equal(cer, cwant.elite_return) and np.array_equal(members, cwant.members)
    assert np.array_equal(ln, tw["L"][rows, idx]) and _same(act, cand[0, rows, idx])
    assert np.array_equal(midx, idx) and _same(mret, bret) and np.array_equal(cidx, idx) and _same(cret, bret)  # one winner
    assert np.abs(nom.astype(np.float64) - want.astype(np.float64)).max() <= tol
    assert (np.abs(ess - wess) / wess <= ess_tol).all()
    assert np.abs(cmean.astype(np.float64) - cwant.mean.astype(np.float64)).max() <= tol
    assert (members.sum(1) == M).all()
    assert eng.solver_cap_hits() == 0
    eng.close()
