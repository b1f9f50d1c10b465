"""emei_evaluate_sequences against the CPU oracle and the NumPy restatement of its header contract (tests/plan_reference.py):
nothing of the HIP library on the expectation's side.  precision="ref" and final_obs everywhere (the float32 mode stays with
the rollout composition of tests/test_gpu_plan.py).  tests/test_plan_reference.py shows on the CPU that the same inputs end
early / run the whole horizon / spread over lengths as each case needs.

On every candidate whose terminal bits the oracle itself can decide (plan_reference.undecidable: at most 1 % are left out):
  length         equal
  |ret - ref|    <= tol_r * sum_{t < L} discount^t * max(|r_t|, 1e-3), tol_r the per-step reward tolerance the rollout kernels are
                 held to against the same oracle (1e-5 CartPole / InvertedPendulum / InvertedDoublePendulum, 1e-4 the multi-step
                 cheetah and Hopper): derived, no new number
  final_obs      rel_err <= 1e-5 against the oracle's observation of step L - 1, wrapped angles on the circle
and no Newton solve may end at the iteration cap."""
import numpy as np
import pytest

import plan_reference as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _engine(*a, **k):
    from emei_amd.engine import Engine

    return Engine(*a, **k)


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_fused_call_vs_oracle_contract(case):
    ref = P.reference(case)
    eng = _engine(case.name, case.N, **case.engine_kw())
    eng.set_state(ref["s0"])
    acts = torch.as_tensor(ref["acts"], device=eng.device)
    ret, L, fo = eng.evaluate_sequences(acts, discount=case.discount, final_obs=True)
    M = case.N * case.K
    ret, L, fo = ret.cpu().numpy().reshape(M), L.cpu().numpy().reshape(M), fo.cpu().numpy().reshape(M, -1)
    wrong, r_ratio, o_ratio = P.compare(case, ref, ret, L, fo)
    worst = f"{case.tag}: ret {r_ratio:.3g} of its bound, final_obs {o_ratio:.3g} of its bound"
    print(worst)
    assert wrong.size == 0, (worst, wrong[:8], L[wrong[:8]], ref["L"][wrong[:8]])
    assert r_ratio <= 1.0, worst
    assert o_ratio <= 1.0, worst
    assert eng.solver_cap_hits() == 0, worst
