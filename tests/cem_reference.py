"""NumPy restatement of emei_plan_cem's elite set and moments (include/emei_hip.h, DESIGN §4 "Planning queries"), written as the
header states them — an explicit comparator for the planner's order, no argsort on floats with NaN — per env, in float64.  Host code
only: the GPU tests hold the kernels to it on the candidates emei_sample_candidates writes and the returns
emei_evaluate_sequences gives them, and tests/test_cem_reference.py holds it to its own edge cases."""
import collections
import functools
import math

import numpy as np

# mean, std float32 [H, N(, act_dim)]; best_return, best_index, elite_return [N]; members bool [N, K]; s2_over_m, std64: the float64
# S2 / M and unrounded std behind `std`, for the tests' error bounds
Cem = collections.namedtuple("Cem", "mean std best_return best_index elite_return members s2_over_m std64")


def _before(ra, ka, rb, kb):
    """the planner's order on (return, k): -1 if a comes before b, 1 if b comes before a"""
    if ra > rb or (math.isnan(rb) and not math.isnan(ra)):
        return -1
    if rb > ra or (math.isnan(ra) and not math.isnan(rb)):
        return 1
    return -1 if ka < kb else (1 if kb < ka else 0)  # neither beats the other: the lower k comes first


def elite_order(returns):
    """[N, K] -> [N, K] int64: per env the candidates in the planner's order — a before b if ret_a > ret_b, or if ret_b is NaN and
    ret_a is not; otherwise the lower k first (so +0.0 and -0.0 tie, NaNs tie with each other and come last, +-inf are ordinary)"""
    r = np.asarray(returns, np.float64)
    out = np.empty(r.shape, np.int64)
    for i in range(r.shape[0]):
        row = [float(x) for x in r[i]]
        out[i] = sorted(range(len(row)), key=functools.cmp_to_key(lambda a, b: _before(row[a], a, row[b], b)))
    return out


def cem(candidates, returns, n_elites, nominal=None, lo=None, hi=None):
    """candidates [H, N, K(, act_dim)] (any dtype; the float32 values of draw_action, 0 / 1 for the discrete envs), returns [N, K],
    nominal [H, N(, act_dim)] float32 or None -> Cem.  Per entry, over the env's elite set E (the first n_elites of elite_order):
        m0 = (double)nominal, or (double)(float32(0.5) * (float32(lo) + float32(hi))) without one (lo = hi = None, the discrete
        envs: 0), d_k = (double)a_k - m0, S1 = sum d_k, S2 = sum d_k^2,
        mean = (float)(m0 + S1 / M),  std = (float)sqrt(max(S2 / M - (S1 / M)^2, 0))"""
    c = np.asarray(candidates).astype(np.float32).astype(np.float64)
    r = np.asarray(returns, np.float64)
    N, K = r.shape
    M = int(n_elites)
    assert 1 <= M <= K
    order = elite_order(r)
    members = np.zeros((N, K), bool)
    for i in range(N):
        members[i, order[i, :M]] = True
    if nominal is not None:
        m0 = np.asarray(nominal, np.float32).astype(np.float64).reshape(c.shape[:2] + c.shape[3:])
    elif lo is not None:
        m0 = np.full(c.shape[:2] + c.shape[3:], float(np.float32(0.5) * (np.float32(lo) + np.float32(hi))))
    else:
        m0 = np.zeros(c.shape[:2] + c.shape[3:])
    mb = members[None, :, :, None] if c.ndim == 4 else members[None, :, :]
    d = (c - np.expand_dims(m0, 2)) * mb  # non-members contribute exact zeros
    s1, s2 = d.sum(2), (d * d).sum(2)
    mu = s1 / M
    var = np.maximum(s2 / M - mu * mu, 0.0)
    std64 = np.sqrt(var)
    rows = np.arange(N)
    return Cem((m0 + mu).astype(np.float32), std64.astype(np.float32), r[rows, order[:, 0]], order[:, 0], r[rows, order[:, M - 1]],
               members, s2 / M, std64)
