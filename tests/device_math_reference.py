"""Inputs and exact references for the device math primitives (tests/test_gpu_device_math.py runs them on the GPU through
tests/device/math_probe.hip; tests/test_device_math_reference.py pins this module itself on the CPU).

References: float64 ops against mpmath (error <= 1e-18 absolute, the 1100-bit reductions of arguments near 1.7e308 included)
or, for bulk points with |x| <= 1e6, numpy.longdouble (x87 extended, eps 1.1e-19); both are returned as longdouble arrays.
float32 ops and Box-Muller against NumPy float64.  Everything is deterministic; references are computed once per process,
shared, and read-only."""
import functools

import mpmath
import numpy as np

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
F64_LIMIT = 1.0e6  # emei_math.h: kFastTrigLimitF64
F32_LIMIT = np.float32(3.0e4)  # kFastTrigLimitF32
TABLE_SIZE = 256
DBL_MAX = np.finfo(np.float64).max
FLT_MAX = np.finfo(np.float32).max
CLOSEST_TO_HALF_PI_MULTIPLE = float(np.ldexp(6381956970095103.0, 797))  # the double closest to a multiple of pi/2


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _signed(v):
    v = np.asarray(v)
    return np.concatenate([v, -v])


def ulp_neighbours(v, k):
    """v and its k neighbours on each side, v an array of floats of one dtype: shape [len(v) * (2k + 1)]"""
    v = np.asarray(v)
    out, up, dn = [v], v, v
    for _ in range(k):
        up, dn = np.nextafter(up, v.dtype.type(np.inf)), np.nextafter(dn, v.dtype.type(-np.inf))
        out += [up, dn]
    return np.concatenate(out)


def decade_points(seed, lo_exp, hi_exp, per_decade, dtype=np.float64, hi_clip=None):
    """per_decade log-uniform magnitudes in each decade [10^e, 10^(e+1)), e = lo_exp .. hi_exp - 1, random signs"""
    rng = np.random.default_rng(seed)
    mag = np.concatenate([10.0 ** rng.uniform(e, e + 1, per_decade) for e in range(lo_exp, hi_exp)])
    if hi_clip is not None:
        mag = np.minimum(mag, hi_clip)
    return (mag * rng.choice([-1.0, 1.0], mag.size)).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the {sin, cos}(k 2pi/256) table: correctly rounded doubles (the specification of abi.hip:emei_trig_table)
@functools.lru_cache(maxsize=None)
def trig_table():
    tab = np.empty((TABLE_SIZE, 2))
    with mpmath.workprec(160):
        for k in range(TABLE_SIZE):
            a = mpmath.mpf(2 * k) / TABLE_SIZE  # in units of pi: the zeros of sin and cos come out as exact zeros
            tab[k] = float(mpmath.sinpi(a)), float(mpmath.cospi(a))  # float(mpf) rounds to nearest
    return _frozen(tab)


def trig_table_host_formula():
    """abi.hip's own formula in this host's long double: (double)sinl(a), (double)cosl(a), a = 2 pi k / 256"""
    a = LD(2) * PI_LD * np.arange(TABLE_SIZE).astype(LD) / LD(TABLE_SIZE)
    return np.stack([np.sin(a).astype(np.float64), np.cos(a).astype(np.float64)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# sin / cos references
def _mp_to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def sincos_mp(x):
    """mpmath sin, cos of float64 x (any magnitude; NaN for non-finite x) as longdouble arrays, error < 1e-19"""
    x = np.asarray(x, np.float64)
    s, c = np.empty(x.shape, LD), np.empty(x.shape, LD)
    with mpmath.workprec(100):  # mpmath raises its working precision by the argument's exponent itself
        for i, v in enumerate(x.tolist()):
            if not np.isfinite(v):
                s[i] = c[i] = np.nan
                continue
            cv, sv = mpmath.cos_sin(mpmath.mpf(v))
            s[i], c[i] = _mp_to_ld(sv), _mp_to_ld(cv)
    return s, c


def sincos_ld(x):
    """long-double libm, for bulk points with |x| <= 1e6"""
    x = np.asarray(x, np.float64)
    assert np.all(np.abs(x) <= F64_LIMIT)
    return np.sin(x.astype(LD)), np.cos(x.astype(LD))


def sincos_ref(x, exact):
    """`exact` marks the points that go through mpmath; the others (|x| <= 1e6) through long double"""
    x, exact = np.asarray(x, np.float64), np.asarray(exact, bool)
    s, c = np.empty(x.shape, LD), np.empty(x.shape, LD)
    s[exact], c[exact] = sincos_mp(x[exact])
    s[~exact], c[~exact] = sincos_ld(x[~exact])
    return s, c


def reduction_residual(x, r):
    """distance of r - x from the nearest multiple of 2 pi, exactly (mpmath at 1300 bits), for finite float64 x, r"""
    out = np.empty(len(x))
    with mpmath.workprec(1300):
        two_pi = 2 * mpmath.pi
        for i, (xv, rv) in enumerate(zip(np.asarray(x, np.float64).tolist(), np.asarray(r, np.float64).tolist())):
            q = (mpmath.mpf(rv) - mpmath.mpf(xv)) / two_pi
            out[i] = float(abs(q - mpmath.nint(q)) * two_pi)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# trig inputs
def tie_points():
    """the neighbourhoods of the table index's ties, (k + 1/2) 2pi/256 +- 3 ulp, both signs: every k of the first period, and 64
    consecutive k near |x| = 1e2, 1e4, 4e5 and just below 1e6"""
    step = LD(2) * PI_LD / LD(TABLE_SIZE)
    ks = [np.arange(TABLE_SIZE)]
    for at in (1e2, 1e4, 4e5, 9.99e5):
        k0 = int(at / float(step))
        ks.append(np.arange(k0, k0 + 64))
    k = np.concatenate(ks).astype(LD)
    centre = ((k + LD(0.5)) * step).astype(np.float64)
    return _signed(ulp_neighbours(centre, 3))


def half_pi_points():
    """multiples of pi/2 +- 2 ulp, both signs: m = 0 .. 64, and 32 consecutive m near |x| = 1e3, 1e5 and just below 1e6"""
    ms = [np.arange(65)]
    for at in (1e3, 1e5, 9.99e5):
        m0 = int(at / float(PI_LD / 2))
        ms.append(np.arange(m0, m0 + 32))
    m = np.concatenate(ms).astype(LD)
    return _signed(ulp_neighbours((m * PI_LD / LD(2)).astype(np.float64), 2))


def limit_points_inside(dtype=np.float64):
    """the fast path's limit and its three neighbours BELOW it, both signs"""
    lim = dtype(F64_LIMIT if dtype is np.float64 else F32_LIMIT)
    v = ulp_neighbours(np.array([lim], dtype), 3)
    return _signed(v[np.abs(v) <= lim])


def limit_points_beyond(dtype=np.float64):
    """... and the three ABOVE it, both signs (the first arguments of the large path)"""
    lim = dtype(F64_LIMIT if dtype is np.float64 else F32_LIMIT)
    v = ulp_neighbours(np.array([lim], dtype), 3)
    return _signed(v[np.abs(v) > lim])


SMALL_SPECIALS_F64 = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308])
SMALL_SPECIALS_F32 = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754944e-38, -1.1754944e-38], np.float32)


def trig_inputs_small_f64():
    """-> (x, exact): |x| <= 1e6.  exact points (mpmath): specials, the limit, the ties, the multiples of pi/2, 100 per decade;
    bulk (long double): 4000 random points per decade 1e-3 .. 1e6"""
    exact = np.concatenate([SMALL_SPECIALS_F64, limit_points_inside(), tie_points(), half_pi_points(),
                            decade_points(11, -3, 6, 100, hi_clip=F64_LIMIT)])
    bulk = decade_points(12, -3, 6, 4000, hi_clip=F64_LIMIT)
    x = np.concatenate([exact, bulk])
    return x, np.arange(x.size) < exact.size


def _exponent_sweep(seed, e_lo, e_hi, dtype):
    """every binary exponent e_lo .. e_hi: the power of two itself, the largest mantissa, 7 random mantissas"""
    rng = np.random.default_rng(seed)
    bits = 52 if dtype is np.float64 else 23
    e = np.arange(e_lo, e_hi + 1)
    frac = rng.integers(1, 2 ** bits - 1, (e.size, 7)).astype(np.float64) / 2.0 ** bits
    mant = np.concatenate([np.ones((e.size, 1)), np.full((e.size, 1), 2.0 - 2.0 ** -bits), 1.0 + frac], axis=1)
    return np.ldexp(mant, e[:, None]).astype(dtype).ravel()


def _finite_abs(v):
    return np.abs(v[np.isfinite(v)])


def trig_inputs_large_f64():
    """finite |x| > 1e6, every point through mpmath: every binary exponent 2^20 .. 2^1023 with 9 mantissas, 2^945 (the
    ldexp(-128) switch) and its neighbours, DBL_MAX, the double closest to a multiple of pi/2, the first doubles beyond the
    limit, one point per decade 1e7 .. 1e308, the finite cold values of the lane tests; negative copies of all of them"""
    pos = np.concatenate([_exponent_sweep(13, 20, 1023, np.float64), ulp_neighbours(np.array([2.0 ** 945]), 1),
                          [DBL_MAX, CLOSEST_TO_HALF_PI_MULTIPLE], np.abs(limit_points_beyond())[:3],
                          np.abs(decade_points(14, 7, 308, 1)), _finite_abs(cold_values())])
    assert np.all(np.isfinite(pos)) and np.all(pos > F64_LIMIT)
    return _signed(pos)


def trig_inputs_small_f32():
    """|x| <= 3e4: specials, the limit, multiples of pi/2 +- 2 ulp, 3000 random points per decade 1e-3 .. 3e4"""
    m = np.concatenate([np.arange(65), np.arange(600, 632), np.arange(19000, 19032)]).astype(np.float64)
    half_pi = _signed(ulp_neighbours((m * np.pi / 2).astype(np.float32), 2))
    half_pi = half_pi[np.abs(half_pi) <= F32_LIMIT]
    return np.concatenate([SMALL_SPECIALS_F32, limit_points_inside(np.float32), half_pi,
                           decade_points(15, -3, 5, 3000, np.float32, hi_clip=float(F32_LIMIT))])


def trig_inputs_large_f32():
    """finite |x| > 3e4: every binary exponent 2^15 .. 2^127 with 9 mantissas, FLT_MAX, the first floats beyond the limit"""
    pos = np.concatenate([_exponent_sweep(16, 15, 127, np.float32), np.array([FLT_MAX], np.float32),
                          np.abs(limit_points_beyond(np.float32))[:3], _finite_abs(cold_values(np.float32))])
    assert np.all(np.isfinite(pos)) and np.all(pos > F32_LIMIT)
    return _signed(pos)


@functools.lru_cache(maxsize=None)
def trig_case(name):
    """{"x", "s", "c"} of one of f64_small, f64_large (longdouble references), f32_small, f32_large (float64 references)"""
    if name == "f64_small":
        x, exact = trig_inputs_small_f64()
        s, c = sincos_ref(x, exact)
    elif name == "f64_large":
        x = trig_inputs_large_f64()
        s, c = sincos_mp(x)
    else:
        x = {"f32_small": trig_inputs_small_f32, "f32_large": trig_inputs_large_f32}[name]()
        s, c = np.sin(x.astype(np.float64)), np.cos(x.astype(np.float64))
    return {"x": _frozen(x), "s": _frozen(s), "c": _frozen(c)}


def abs_err(got, ref):
    """max |got - ref| in the reference's precision; a NaN on one side only is an infinite error"""
    got, ref = np.asarray(got), np.asarray(ref)
    wide = ref.dtype if ref.dtype == LD else np.float64
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(wide) - ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    d = np.where(both_nan, 0, np.where(np.isnan(d), np.inf, d))
    return float(d.max()) if d.size else 0.0


def rel_err(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    wide = ref.dtype if ref.dtype == LD else np.float64
    with np.errstate(all="ignore"):
        d = np.abs((got.astype(wide) - ref) / ref)
    d = np.where(np.isnan(d), np.inf, d)
    return float(d.max()) if d.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# lane layouts of the cold-path tests: the position of a value in the array is the lane it runs in (64 lanes per wave, 4 waves
# per block).  Every layout starts with the same 8 waves; the ragged ones add a partial last block.
WAVE = 64
WAVE_PATTERNS = ("cold_lane_0", "cold_lane_31", "cold_lane_63", "alternating_even", "alternating_odd", "all_cold_but_one", "fully_cold",
                 "all_hot")
RAGGED_TAILS = (1, 63, 65)


def _wave_mask(pattern):
    lane = np.arange(WAVE)
    return {"cold_lane_0": lane == 0, "cold_lane_31": lane == 31, "cold_lane_63": lane == 63, "alternating_even": lane % 2 == 0,
            "alternating_odd": lane % 2 == 1, "all_cold_but_one": lane != 17, "fully_cold": lane >= 0, "all_hot": lane < 0}[pattern]


def cold_layouts():
    """-> [(name, cold mask)]: the 8 wave patterns as two full blocks, and for each ragged tail (n % 256 in {1, 63, 65}) the same
    followed by a partial block whose lanes alternate, starting cold and starting hot"""
    full = np.concatenate([_wave_mask(p) for p in WAVE_PATTERNS])
    out = [("full_blocks", full)]
    for tail in RAGGED_TAILS:
        for first_cold in (True, False):
            t = (np.arange(tail) % 2 == 0) == first_cold
            out.append((f"ragged_{tail}_{'cold' if first_cold else 'hot'}_first", np.concatenate([full, t])))
    return out


LAYOUT_MAX_N = len(WAVE_PATTERNS) * WAVE + max(RAGGED_TAILS)


def mix(hot, cold, mask):
    """hot[:n] with the masked positions replaced by the cold values in turn"""
    x = np.array(hot[: mask.size], copy=True)
    x[mask] = np.resize(cold, int(mask.sum()))
    return x


def hot_values(dtype=np.float64):
    """LAYOUT_MAX_N in-range arguments: the limit itself, ties, multiples of pi/2, random points of every decade"""
    if dtype is np.float64:
        pool = np.concatenate([limit_points_inside(), tie_points()[::97], half_pi_points()[::53], decade_points(21, -3, 6, 60, hi_clip=F64_LIMIT)])
    else:
        pool = np.concatenate([limit_points_inside(np.float32), decade_points(22, -3, 5, 80, np.float32, hi_clip=float(F32_LIMIT))])
    assert pool.size >= LAYOUT_MAX_N
    return _frozen(pool[:LAYOUT_MAX_N])


def cold_values(dtype=np.float64):
    """arguments of the cold path: just beyond the limit, large, huge, +-inf, NaN"""
    if dtype is np.float64:
        return np.array([np.nextafter(F64_LIMIT, np.inf), -3.3e7, np.inf, 1e300, np.nan, -np.inf, 2.0 ** 945, -DBL_MAX, 7.7e8, -1.0000001e6,
                         CLOSEST_TO_HALF_PI_MULTIPLE])
    return np.array([np.nextafter(F32_LIMIT, np.float32(np.inf)), -3.3e7, np.inf, 3e38, np.nan, -np.inf, 1e10, -FLT_MAX, 7.7e8, -30001.0], np.float32)


def wrap_cold_values(dtype=np.float64):
    """angles whose wrap takes the fix-up branch (|o| >= pi or NaN after the first estimate): non-finite, far beyond the
    domain, and one ulp below -pi (the quotient estimate is one period off)"""
    t = dtype
    return np.array([np.nan, np.inf, -np.inf, np.finfo(t).max, -np.finfo(t).max, 1e300 if t is np.float64 else 1e30,
                     np.nextafter(t(-np.pi), t(-np.inf))], t)


# ---------------------------------------------------------------------------------------------------------------------------
# reciprocals: the ranges of tools/rcp_accuracy.hip
def rcp_inputs(dtype=np.float64):
    rng = np.random.default_rng(31)
    lin = rng.uniform(0.05, 20.0, 20000)
    log = 2.0 ** rng.uniform(-20, 20, 20000)
    edge = np.concatenate([2.0 ** np.arange(-20, 21), [0.05, 20.0, 3.0, 1.0 / 3, 0.1, 10.0, 1 - 2.0 ** -53, 1 + 2.0 ** -52]])
    return _signed(np.concatenate([edge, lin, log])).astype(dtype)


def div_inputs(dtype=np.float64):
    d = rcp_inputs(dtype)
    rng = np.random.default_rng(32)
    n = (10.0 ** rng.uniform(-3, 3, d.size) * rng.choice([-1.0, 1.0], d.size)).astype(dtype)
    n[:4] = dtype(1e-3), dtype(-1e-3), dtype(1e3), dtype(-1e3)
    return n, d


def rsqrt_inputs(dtype=np.float64):
    rng = np.random.default_rng(33)
    x = np.concatenate([10.0 ** rng.uniform(-20, 6, 40000), 4.0 ** np.arange(-30, 10), [1e-20, 1e6, 2.0, 3.0, 0.5]])
    return x.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# angle wrap
WRAP_F64_DOMAIN = 1e15  # bit-equal to NumPy up to here (the quotient estimate is exact below ~1e16)
WRAP_F32_DOMAIN = 1e6


def wrap_boundary_points(dtype=np.float64):
    pi = np.pi
    base = np.array([0.0, pi, -pi, 3 * pi, -3 * pi, 2 * pi, -2 * pi, 101 * pi, -101 * pi, 600.0, -600.0, 1e5 * pi, -1e5 * pi, 12345 * pi,
                     -99999 * pi])
    if dtype is np.float64:
        base = np.concatenate([base, [1e9 * pi, -(1e12 + 1) * pi, 3e14 * pi]])
        return np.concatenate([ulp_neighbours(base, 2), base + 1e-9, base - 1e-9])
    return ulp_neighbours(base.astype(np.float32), 2)


def wrap_inputs_in_domain(dtype=np.float64):
    if dtype is np.float64:
        bulk = decade_points(41, -3, 15, 2500, hi_clip=WRAP_F64_DOMAIN)
        return np.concatenate([SMALL_SPECIALS_F64, wrap_boundary_points(), [WRAP_F64_DOMAIN, -WRAP_F64_DOMAIN], bulk])
    bulk = decade_points(42, -3, 6, 5000, np.float32, hi_clip=WRAP_F32_DOMAIN)
    return np.concatenate([SMALL_SPECIALS_F32, wrap_boundary_points(np.float32), np.array([WRAP_F32_DOMAIN, -WRAP_F32_DOMAIN], np.float32), bulk])


def wrap_inputs_anywhere(dtype=np.float64):
    """the domain's inputs plus everything beyond it: every decade up to the format's maximum, the maximum, +-inf, NaN"""
    top = 308 if dtype is np.float64 else 38
    with np.errstate(over="ignore"):
        far = decade_points(43, 15 if dtype is np.float64 else 6, top, 200).astype(dtype)
    far = far[np.isfinite(far)]
    mx = np.finfo(dtype).max
    return np.concatenate([wrap_inputs_in_domain(dtype), far, np.array([mx, -mx, np.inf, -np.inf, np.nan], dtype)])


def wrap_reference(theta):
    """inverted_pendulum.py:45-49 in the dtype of theta: (theta + pi) % (2 pi) - pi with NumPy's floored modulo"""
    t = theta.dtype.type
    pi = t(3.141592653589793)
    with np.errstate(all="ignore"):
        return (theta + pi) % (t(2) * pi) - pi


def same_wrap(got, ref):
    """bit for bit — except on the wrap point itself, where NumPy's own remainder can round up to the modulus (theta one ulp
    below -pi gives +pi there, -pi on the device: the same angle, one representative each; tests/test_gpu_invpend.py:
    test_angle_wrap_at_its_boundaries accepts the same)"""
    pi = np.pi
    at_wrap = (np.abs(np.abs(got.astype(np.float64)) - pi) < 1e-6) & (np.abs(np.abs(ref.astype(np.float64)) - pi) < 1e-6)
    return (got == ref) | at_wrap


# ---------------------------------------------------------------------------------------------------------------------------
# random numbers
def philox_numpy(seed, env, episode, block):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised: key = seed, counter = (env lo, env hi, episode, block) -> [n, 4] uint32"""
    env = np.asarray(env, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = env & m32, env >> np.uint64(32)
    c2, c3 = np.asarray(episode, np.uint64) & m32, np.asarray(block, np.uint64) & m32
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & m32, n2, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


# known answers of the Random123 distribution (kat_vectors): counter, key -> output
PHILOX_KAT = (
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)

PHILOX_SEEDS = (0, 1, 0x5EED, 0xFFFFFFFF, 0x1_0000_0000, 0xDEADBEEF_00000000, 0x299F31D0_A4093822, 0xFFFFFFFF_FFFFFFFF)


def philox_cases():
    """-> env [n] uint64, episode [n] uint32, block [n] uint32: the edges (env 0, 2^32 - 1, 2^32, 2^63, 2^64 - 1; episode and block
    0, 1, 0xFFFFFFFF) crossed, and random words with the high bits set"""
    rng = np.random.default_rng(51)
    env_e = np.array([0, 1, 63, 64, 0xFFFFFFFF, 0x1_0000_0000, 0x1_0000_0001, 1 << 63, 0xFFFFFFFF_FFFFFFFF], np.uint64)
    w_e = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)
    e, p, b = np.meshgrid(env_e, w_e, w_e, indexing="ij")
    n = 300
    env = np.concatenate([e.ravel(), rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)])
    episode = np.concatenate([p.ravel(), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)])
    block = np.concatenate([b.ravel(), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)])
    return env, episode, block


def philox_oracle(seed, env, episode, block):
    """the same through oracle.philox, the restatement the env tests already trust"""
    from oracle import oracle as O

    return np.stack([O.philox(int(seed), int(e), int(p), int(b)) for e, p, b in zip(env.tolist(), episode.tolist(), block.tolist())])


def u01_reference(r):
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


BM_FIELDS = 1 << 24
BM_FIXED_B_FIELDS = (0, 1, 0x555555, BM_FIELDS - 1)  # angle 0, the smallest, about a third of a turn, the largest
BM_MAX_RADIUS = float(np.sqrt(48 * np.log(2.0)))  # u1 = 2^-24


def boxmuller_radius(a_field):
    """sqrt(-2 ln u1), u1 = (field + 1) / 2^24 in (0, 1] (oracle/integrators.h), float64"""
    u1 = (np.asarray(a_field, np.float64) + 1.0) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1))


def boxmuller_direction(b_field):
    """(cos, sin)(2 pi t), t = field / 2^24 turns, float64"""
    ang = 2.0 * np.pi * (np.asarray(b_field, np.float64) * 2.0 ** -24)
    return np.cos(ang), np.sin(ang)
