"""NumPy restatement of the candidate specification of emei_plan_shooting / emei_sample_candidates (include/emei_hip.h,
DESIGN §4 "Planning queries") and of the planner's order.  Host code only: the GPU tests hold the kernels to it, and
tests/test_shooting_reference.py holds it to the oracle's Philox, the Random123 known answer and its own edge cases."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, g, k, block):
    """Philox4x32-10 (Salmon et al., SC'11): key = the 64-bit seed, counter = (g lo, g hi, k, block), broadcast -> [..., 4] uint32"""
    g, k, block = np.broadcast_arrays(np.asarray(g, np.uint64), np.asarray(k, np.uint64), np.asarray(block, np.uint64))
    c0, c1, c2, c3 = g & M32, g >> np.uint64(32), k & M32, block & M32
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, g, k, n_words):
    """W[m] = philox4x32_10(seed, g, k, m >> 2).v[m & 3] for m < n_words: g [N], k [K] -> [n_words, N, K] uint32"""
    g, k = np.asarray(g, np.uint64), np.asarray(k, np.uint64)
    nb = (n_words + 3) // 4
    blk = philox4x32_10(seed, g[None, :, None], k[None, None, :], np.arange(nb, dtype=np.uint64)[:, None, None])  # [nb, N, K, 4]
    return np.moveaxis(blk, -1, 1).reshape(nb * 4, len(g), len(k))[:n_words]


def field(w):
    """the 24-bit field w >> 8 both u01 and boxmuller read"""
    return np.asarray(w, np.uint32) >> np.uint32(8)


def u01(w):
    """(w >> 8) * 2^-24 in [0, 1): exact in float32"""
    return field(w).astype(np.float32) * np.float32(2.0 ** -24)


def discrete(seed, g, K, H, prob=None):
    """[H, N, K] uint8: u(W[t]) < p, p = 0.5 or prob[t, i] (float32)"""
    u = u01(words(seed, g, np.arange(K), H))
    p = np.float32(0.5) if prob is None else np.asarray(prob, np.float32)[:, :, None]
    return (u < p).astype(np.uint8)


def discrete_top_bit(seed, g, K, H):
    """the p = 0.5 rule stated on the word itself: 1 - the top bit of W[t]"""
    return (1 - (words(seed, g, np.arange(K), H) >> np.uint32(31))).astype(np.uint8)


def uniform(seed, g, K, H, act_dim, lo, hi):
    """[H, N, K, act_dim] float32: fmaf(u(W[t * act_dim + a]), hi - lo, lo) — lo + (hi - lo) * u is exact in float64 (a 24-bit
    field times a small integer, plus a small integer), so one rounding to float32 is what the fused operation gives"""
    u = u01(words(seed, g, np.arange(K), H * act_dim)).astype(np.float64)  # [H * A, N, K]
    v = (float(lo) + (float(hi) - float(lo)) * u).astype(np.float32)
    return np.moveaxis(v.reshape(H, act_dim, len(g), K), 1, -1)


def gaussian_exact(seed, g, K, H, act_dim, lo, hi, mean, sigma):
    """[H, N, K, act_dim] float64, unrounded: clip(mean + float32(sigma) * z, lo, hi) with the EXACT Box-Muller normal of the spec —
    c = t * act_dim + a, q = c >> 1, u1 = (field(W[2q]) + 1) / 2^24, turns = field(W[2q + 1]) / 2^24, z = sqrt(-2 ln u1) *
    (cos, sin)(2 pi turns)[c & 1]"""
    n = H * act_dim
    w = words(seed, g, np.arange(K), n + (n & 1))
    a, b = field(w[0::2]).astype(np.float64), field(w[1::2]).astype(np.float64)  # [ceil(n / 2), N, K]
    rad = np.sqrt(-2.0 * np.log((a + 1.0) * 2.0 ** -24))
    ang = 2.0 * np.pi * (b * 2.0 ** -24)
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).reshape(-1, len(g), K)[:n]  # c = 2q + (c & 1)
    z = np.moveaxis(z.reshape(H, act_dim, len(g), K), 1, -1)
    m = np.asarray(mean, np.float32).astype(np.float64).reshape(H, len(g), 1, act_dim)
    return np.clip(m + float(np.float32(sigma)) * z, float(lo), float(hi))


def best_of(returns):
    """[N, K] -> k* [N]: a beats b if ret_a > ret_b, or if ret_b is NaN and ret_a is not; otherwise the lower k wins.  Written as
    the sequential scan the rule describes, not as argmax."""
    r = np.asarray(returns, np.float64)
    best = np.zeros(r.shape[0], np.int64)
    for i in range(r.shape[0]):
        for k in range(1, r.shape[1]):
            a, b = r[i, k], r[i, best[i]]
            if a > b or (np.isnan(b) and not np.isnan(a)):
                best[i] = k
    return best
