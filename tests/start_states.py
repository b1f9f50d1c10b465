"""Start-state draws shared by the family one-step tests (tests/test_gpu_invpend.py, test_gpu_cheetah.py, test_gpu_hopper.py) and the
kernel matrix (tests/kernel_matrix.py).  A helper module: NumPy only, no fixtures, no test."""
import numpy as np


def invpend_states(rng, n):
    s = np.empty((n, 4))
    s[:, 0] = rng.uniform(-2.3, 2.3, n)  # beyond the +-2 rail on purpose: limit force engaged
    s[:, 1] = rng.uniform(-12, 12, n)
    s[:, 2] = rng.normal(0, 2, n)
    s[:, 3] = rng.normal(0, 5, n)
    s[: n // 4] = rng.standard_normal((n // 4, 4)) * 5e-3
    return s


def cheetah_states(rng, n):
    """flight, standing, crouched into the floor (many contacts), joints pushed past their limits"""
    q = rng.normal(0, 0.15, (n, 9))
    q[:, 1] = rng.uniform(-0.35, 0.3, n)
    q[:, 2] = rng.normal(0, 0.4, n)
    q[: n // 4, 3:] = rng.uniform(-1.3, 1.3, (n // 4, 6))
    v = rng.normal(0, 1.5, (n, 9))
    return np.concatenate([q, v], axis=1)


def hopper_states(rng, n):
    """flight, standing on the foot, pressed into the floor (several contacts), joints past their limits, lying"""
    q = rng.normal(0, 0.1, (n, 6))
    q[:, 1] = 1.25 + rng.uniform(-0.08, 0.3, n)
    q[:, 3:5] = -np.abs(rng.normal(0, 0.3, (n, 2)))
    k = n // 5
    q[:k, 3:] = rng.uniform(-3.0, 0.5, (k, 3))           # limits
    q[k : 2 * k, 1] = rng.uniform(0.0, 0.3, k)           # lying / deep contact
    q[k : 2 * k, 2] = rng.uniform(-1.7, 1.7, k)
    v = rng.normal(0, 1.5, (n, 6))
    return np.concatenate([q, v], axis=1)
