"""NumPy restatement of emei_plan_mppi's weight rule and outputs (include/emei_hip.h, DESIGN §4 "Planning queries"), written as
the case analysis the header gives, per env and per candidate, in float64 — not as a soft-max.  Host code only: the GPU tests hold
the kernels to it on the candidates emei_sample_candidates writes and the returns emei_evaluate_sequences gives them, and
tests/test_mppi_reference.py holds it to its own edge cases."""
import math

import numpy as np

from shooting_reference import best_of


def weights(returns, temperature):
    """[N, K] float64 returns -> (w [N, K] float64, k* [N]): per env, with (k*, r*) the planner's winner,
        r* is NaN (every return is NaN)                      w_k = 1 for all k
        otherwise, r_k is NaN                                w_k = 0
        otherwise, r_k == r* (a +-inf maximum and all ties)  w_k = 1
        otherwise                                            w_k = exp((r_k - r*) / temperature)   (-inf gives 0)"""
    r = np.asarray(returns, np.float64)
    T = float(temperature)
    best = best_of(r)
    w = np.empty_like(r)
    for i in range(r.shape[0]):
        rs = r[i, best[i]]
        for k in range(r.shape[1]):
            rk = r[i, k]
            if math.isnan(rs):
                w[i, k] = 1.0
            elif math.isnan(rk):
                w[i, k] = 0.0
            elif rk == rs:
                w[i, k] = 1.0
            elif rk == -math.inf:
                w[i, k] = 0.0
            else:
                w[i, k] = math.exp((rk - rs) / T)  # rk < rs, both finite or rs = +inf: the argument is <= 0 (or -inf)
    return w, best


def mppi(candidates, returns, temperature):
    """candidates [H, N, K(, act_dim)] (any dtype; the float32 values of draw_action, 0 / 1 for the discrete envs), returns [N, K]
    -> (nominal_out float32 [H, N(, act_dim)], best_return float64 [N], best_index [N], ess float64 [N]):
        Z = sum_k w_k (>= 1),  nominal_out[t, i(, a)] = (float32)(sum_k w_k * (double)action_k[t, i(, a)] / Z),  ess = Z^2 / sum_k w_k^2"""
    c = np.asarray(candidates).astype(np.float32).astype(np.float64)
    r = np.asarray(returns, np.float64)
    w, best = weights(r, temperature)
    Z = w.sum(1)
    wb = w[None, :, :, None] if c.ndim == 4 else w[None, :, :]
    num = (c * wb).sum(2)
    Zb = Z[None, :, None] if c.ndim == 4 else Z[None, :]
    out = (num / Zb).astype(np.float32)
    ess = Z * Z / (w * w).sum(1)
    return out, r[np.arange(r.shape[0]), best], best, ess
