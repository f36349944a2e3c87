"""Argument sets for the deterministic fp32 functions, shared by tests/test_math_accuracy_host.py (the oracle and the
NumPy twins against float64, CPU) and tests/test_gpu_math_probe.py (the device against the oracle, the twins and IEEE arithmetic), and the
error measures the two modules print.  Every set is a float32 array built from bit patterns, sorted and without repeats; each is built
once and then shared read-only."""
import ctypes as C
import functools

import numpy as np

F = np.float32
TWIN_CAP = 200000          # the most a set routed through the frompyfunc-based NumPy twins (policy_sample._fmaf) may hold
U_MAX = F(1) - F(2.0 ** -24)                                   # csrc/eb_policy_logp_device.h:U_MAX
HEADING_F16_MAX = F(F(65504) * F(np.pi)) / F(180)              # deg2rad of the largest finite binary16 heading (one rounding per op)
SQRT_HALF_MANT = 0x3504f3                                      # mantissa bits of float32(sqrt(1/2)): log_det's split


def _frozen(a):
    a.setflags(write=False)
    return a


def from_bits(bits):
    """sorted, repeat-free uint32 patterns -> the read-only float32 array"""
    return _frozen(np.unique(np.asarray(bits, np.uint64).astype(np.uint32)).view(F))


def bits_of(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def around(values, span=64, both_signs=True):
    """the bit patterns within +-span of float32(values) (and of their negatives), clipped to the pattern range of each sign"""
    b = bits_of(np.atleast_1d(np.asarray(values, np.float64)).astype(F)).astype(np.int64) & 0x7fffffff
    p = np.clip(b[:, None] + np.arange(-span, span + 1)[None, :], 0, 0x7fffffff).reshape(-1)
    return np.concatenate([p, p | 0x80000000]) if both_signs else p


SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000,             # +-0, +-inf
                         0x7fc00000, 0xffc00000, 0x7fc12345, 0xffe00001,             # quiet NaNs: both signs, with payloads
                         0x00000001, 0x80000001, 0x007fffff, 0x807fffff,             # the smallest and largest subnormal
                         0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff], np.int64)  # FLT_MIN, FLT_MAX


@functools.lru_cache(None)
def stride_bits():
    """a stride-4099 sample of all 2^32 patterns (about 1 M), as tests/test_exact_math.py draws it"""
    return np.arange(0, 1 << 32, 4099, dtype=np.int64)


@functools.lru_cache(None)
def boundary_bits():
    """+-4096 patterns around every exponent boundary, both signs"""
    e = (np.arange(1, 255, dtype=np.int64) << 23)[:, None] + np.arange(-4096, 4097, dtype=np.int64)[None, :]
    p = np.clip(e.reshape(-1), 0, 0x7f7fffff)
    return np.concatenate([p, p | 0x80000000])


@functools.lru_cache(None)
def common():
    """what every function sees: the specials, the stride sample of all patterns and the exponent boundaries (about 5 M)"""
    return from_bits(np.concatenate([SPECIAL_BITS, stride_bits(), boundary_bits()]))


@functools.lru_cache(None)
def common_capped():
    """a thinned common() for the NumPy twins: the specials, every 37th of the stride sample, +-16 patterns around every exponent boundary"""
    e = (np.arange(1, 255, dtype=np.int64) << 23)[:, None] + np.arange(-16, 17, dtype=np.int64)[None, :]
    p = np.clip(e.reshape(-1), 0, 0x7f7fffff)
    return from_bits(np.concatenate([SPECIAL_BITS, stride_bits()[::37], p, p | 0x80000000]))


def _extras(name):
    if name == 'sincos':
        k = np.arange(0, 1025, dtype=np.float64) * (np.pi / 2)          # every float within +-64 patterns of k * pi/2, k <= 1024
        return np.concatenate([around(k), around([float(HEADING_F16_MAX), 2.0 ** 16 * np.pi / 2, 2.0 ** 31 * np.pi / 2]),
                               around([3e9, 4e9, 1e10], 0)])
    if name == 'atan':
        return np.concatenate([around([0.4142135623730950, 2.414213562373095]), [0x3edf657f, 0xbedf657f]])
    if name == 'exp':
        n = np.arange(-127, 129, dtype=np.float64)                      # where rint(x * log2 e) changes: x = (n + 1/2) ln 2
        return around(np.concatenate([[-87.0, 88.0], (n + 0.5) * np.log(2.0)]))
    if name == 'tanh':
        return around([0.625, 44.0])
    if name == 'log':
        m = (np.arange(1, 255, dtype=np.int64) << 23 | SQRT_HALF_MANT)[:, None] + np.arange(-64, 65, dtype=np.int64)[None, :]
        sub = np.arange(1, 1 << 23, 65521, dtype=np.int64)              # subnormals and negatives: outside the domain, pinned
        return np.concatenate([m.reshape(-1), around([1.0, 2.0 ** -24, 2.0], both_signs=False), sub, sub | 0x80000000,
                               around([1.0, 0.5, 3.0], 0)])
    if name == 'artanh':
        lo, hi = int(bits_of(F(2.0 ** -30))[0]), int(bits_of(U_MAX)[0])
        p = np.concatenate([np.arange(lo, hi, 2741, dtype=np.int64), np.arange(hi - 4096, hi + 1, dtype=np.int64),
                            np.arange(lo, lo + 65, dtype=np.int64)])
        return np.concatenate([p, p | 0x80000000, [0, 0x80000000, 0x7fc00000]])
    raise KeyError(name)


@functools.lru_cache(None)
def full(name):
    """the set of `name` ('sincos', 'atan', 'exp', 'tanh'): common() and the function's own points — a few million values, for the oracle
    and the device"""
    return from_bits(np.concatenate([bits_of(common()).astype(np.int64), _extras(name)]))


@functools.lru_cache(None)
def capped(name):
    """the set of `name` for the NumPy twins (at most TWIN_CAP values): common_capped() and the function's own points, thinned where they
    are many.  'log' and 'artanh' have no other set: their only CPU twin is the NumPy one."""
    ex = np.asarray(_extras(name), np.int64)
    if name == 'sincos':                                                # every 8th multiple of pi/2 keeps its +-64 patterns
        k = np.arange(0, 1025, 8, dtype=np.float64) * (np.pi / 2)
        ex = np.concatenate([around(k), around([float(HEADING_F16_MAX), 2.0 ** 16 * np.pi / 2, 2.0 ** 31 * np.pi / 2]),
                             around([3e9, 4e9, 1e10], 0)])
    base = SPECIAL_BITS if name == 'artanh' else bits_of(common_capped()).astype(np.int64)
    s = from_bits(np.concatenate([base, ex]))
    assert s.size <= TWIN_CAP, (name, s.size)
    return s


# ---- IEEE operations: dividends, divisor pairs ----
@functools.lru_cache(None)
def div_pairs():
    """(x, y) for x / y: the stride sample against a fixed shuffle of itself, the specials against each other, and quotients that land
    in and around the subnormal range (a small dividend over a large divisor)"""
    rng = np.random.default_rng(20240607)
    x = common()[::5]
    y = x[rng.permutation(x.size)]
    sp = SPECIAL_BITS.astype(np.uint32).view(F)
    sx, sy = [t.reshape(-1) for t in np.meshgrid(sp, sp)]
    tx = (rng.integers(0x00800000, 0x0d000000, 200000).astype(np.uint32)).view(F)       # 2^-126 .. 2^-101
    ty = (rng.integers(0x3f800000, 0x4b800000, 200000).astype(np.uint32)).view(F)       # 1 .. 2^24
    ux = (rng.integers(0x00000001, 0x00800000, 100000).astype(np.uint32)).view(F)       # subnormal dividends
    uy = (rng.integers(0x3e000000, 0x41000000, 100000).astype(np.uint32)).view(F)       # 1/8 .. 8
    sign = np.where(rng.integers(0, 2, 300000) == 1, F(-1), F(1))
    X = np.concatenate([x, sx, np.concatenate([tx, ux]) * sign])
    Y = np.concatenate([y, sy, ty, uy])
    return _frozen(np.ascontiguousarray(X, F)), _frozen(np.ascontiguousarray(Y, F))


# ---- the counter-based uniforms: splitmix64 and its inverse on Python integers ----
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def splitmix64(z):
    """csrc/eb_env_device.h:splitmix64 on a Python integer"""
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * _C1) & M64
    z = ((z ^ (z >> 27)) * _C2) & M64
    return z ^ (z >> 31)


def splitmix64_inverse(out):
    """the z with splitmix64(z) == out: each step of the mix is a bijection of the 64-bit integers"""
    z = out ^ (out >> 31) ^ (out >> 62)
    z = (z * pow(_C2, -1, 1 << 64)) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * pow(_C1, -1, 1 << 64)) & M64
    z = z ^ (z >> 30) ^ (z >> 60)
    return (z - GOLDEN) & M64


def key_with_uniform(top24, index, low40=0x5a5a5a5a5a):
    """a key whose uniform number `index` (csrc/eb_env_device.h:u01(key, index)) has exactly the given top 24 bits, so is top24 * 2^-24"""
    return (splitmix64_inverse(((top24 & 0xffffff) << 40) | (low40 & 0xffffffffff)) - GOLDEN * index) & M64


def seed_of_key(key):
    """the seed with which policy_sample.policy_noise_reference(…, seed, counter=0) derives this key (key = splitmix64(seed))"""
    return splitmix64_inverse(key)


# Keys whose uniforms 0 AND 1 are both fixed (normal_pair's pair 0 of row 0 reads exactly these two): found by trying the free low 40 bits of
# the first output until the second lands too (one in 2^24 does); the tests re-derive both uniforms from each key before they use it.
#   first uniform 0 (u = 1, radius 0) with the second 0; first uniform 1 - 2^-24 (u = 2^-24, the largest radius) with the second 0
JOINT_KEYS = ((0x7382290d7c81a8b3, 'first uniform 0 and second uniform 0: u = 1, v = 0'),
              (0x7013606d295d0ac0, 'first uniform 1 - 2^-24 and second uniform 0: u = 2^-24, v = 0'))
JOINT_UNIFORMS = ((0, 0), (0xffffff, 0))      # the top 24 bits of uniforms 0 and 1 under each of JOINT_KEYS


@functools.lru_cache(None)
def extreme_keys():
    """[(key, what)]: the constructed extremes of normal_pair's pair 0 of row 0"""
    keys = [(key_with_uniform(0, 0), 'first uniform 0: u = 1'),
            (key_with_uniform(0xffffff, 0), 'first uniform 1 - 2^-24: u = 2^-24'),
            (key_with_uniform(0, 1), 'second uniform 0'),
            (key_with_uniform(0xffffff, 1), 'second uniform 1 - 2^-24')]
    return keys + list(JOINT_KEYS)


# ---- binary16 ----
@functools.lru_cache(None)
def f16_set():
    """floats for the float -> half store: every half's value, every rounding tie between neighbouring halves with the pattern on either
    side of it, the overflow threshold 65520, the subnormal-half range and below it, and a thinned common()"""
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)        # the finite non-negative halves, ascending
    h = np.append(h, 65536.0)                                                            # the value the exponent after the last would have
    ties = bits_of(((h[:-1] + h[1:]) / 2).astype(F)).astype(np.int64)                   # exact in float32
    t3 = (ties[:, None] + np.arange(-1, 2)[None, :]).reshape(-1)
    vals = bits_of(np.arange(0, 1 << 16, dtype=np.uint16).view(np.float16).astype(F)).astype(np.int64)
    sub = np.arange(int(bits_of(F(2.0 ** -27))[0]), int(bits_of(F(2.0 ** -13))[0]), 1543, dtype=np.int64)
    return from_bits(np.concatenate([t3, t3 | 0x80000000, vals, sub, sub | 0x80000000, around([65504.0, 65520.0, 65536.0, 2.0 ** -24,
                                     2.0 ** -25, 2.0 ** -14]), bits_of(common()[::3]).astype(np.int64)]))


# ---- the CPU twins ----
def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_fn(name, x):
    """eb_oracle_<name>f over a float32 array -> float32 array(s)"""
    from tests._helpers import oracle_lib
    lib = oracle_lib().lib
    x = np.ascontiguousarray(x, F)
    fn = getattr(lib, 'eb_oracle_%sf' % name)
    fn.restype = None
    if name == 'sincos':
        s, c = np.empty_like(x), np.empty_like(x)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        fn(_fp(x), _fp(s), _fp(c), x.size)
        return s, c
    y = np.empty_like(x)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    fn(_fp(x), _fp(y), x.size)
    return y


def artanh_twin(u):
    """csrc/eb_policy_logp_device.h:artanh_log from the twin of log_det"""
    from env_build_amd import policy_sample as _PS
    u = np.ascontiguousarray(u, F)
    with np.errstate(all='ignore'):
        return (F(0.5) * (_PS._log_det(F(1) + u) - _PS._log_det(F(1) - u))).astype(F)


# ---- error measures ----
def ulp_of(ref):
    """one unit in the last place of float32 at |ref| (float64 array): 2^(floor(log2 |ref|) - 23), never below 2^-149"""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def worst(got, ref, x=None):
    """-> (largest error in ulps of the result, largest absolute error, the argument at the largest ulp error) of float32 `got` against
    float64 `ref`, over the entries where both are finite"""
    got64 = np.asarray(got, np.float64)
    ok = np.isfinite(got64) & np.isfinite(ref)
    if not ok.any():
        return 0.0, 0.0, None
    err = np.abs(got64[ok] - ref[ok])
    u = err / ulp_of(ref[ok])
    i = int(np.argmax(u))
    return float(u[i]), float(err.max()), (None if x is None else np.asarray(x)[ok][i])


ACCURACY_LOG = {}     # 'function, domain' -> (max ulp, max abs, at, n): what test_math_accuracy_host.py measured, printed by it


def same_bits(got_bits, want, what, nan_bits=False):
    """device bits == reference bits elementwise.  nan_bits False: where the reference is a NaN the device's must be a NaN, and its bits
    are not compared (IEEE 754 leaves the sign of a generated NaN and the payload an operation passes on to the implementation, and x86
    and a C library's fmaf choose differently); True: NaNs are compared bit for bit too (against the oracle, and where the function
    returns its argument by a select)."""
    g = np.asarray(got_bits, np.uint32)
    w = np.ascontiguousarray(want).view(np.uint32) if np.asarray(want).dtype != np.uint32 else np.asarray(want)
    assert g.shape == w.shape, '%s: shape %s vs %s' % (what, g.shape, w.shape)
    bad = g != w
    if not nan_bits:
        gn, wn = np.isnan(g.view(F)), np.isnan(w.view(F))
        bad = np.where(wn | gn, gn != wn, bad)
    n = int(bad.sum())
    if n:
        i = int(np.argmax(bad))
        raise AssertionError('%s: %d of %d differ; first at index %d: got 0x%08x, want 0x%08x' % (what, n, g.size, i, g[i], w[i]))
