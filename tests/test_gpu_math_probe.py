"""The deterministic fp32 functions evaluated ON THE DEVICE (tests/_math_probe.hip: the product's headers, the product's compiler flags),
over the argument sets of tests/_math_sets.py, held bit for bit to

  * the CPU oracle's eb_sincosf / eb_atanf / eb_expf / eb_tanhf (tests/test_math_accuracy_host.py holds those to float64),
  * the NumPy twins of policy_sample (on the capped sets; log_det, artanh_log, u01 and normal_pair have no other CPU text),
  * each other (sincos_det_k == sincos_det, elu_det == exp_det - 1),
  * IEEE arithmetic as the host performs it in float32 (div_const / div_by / deg2rad / rad2deg, x / y, 1 / x, sqrtf, float <-> binary16).

Against the oracle every bit is compared, the sign and payload of a NaN included: sincos(+-inf) and sincos / atan / tanh of a NaN come out
of the same operations in the same order on both sides, and the GPU and the host's FPU agree on them.  Where bits of a NaN are NOT compared, and only "a NaN for a NaN" is held (_math_sets.same_bits):
  * the NumPy twins of sincos, tanh and artanh: their fmaf is libm's, called element by element; which of two NaN operands an x86 fused
    multiply-add passes on depends on the instruction form the C library's build chose, which IEEE 754 leaves open — 115 patterns of the
    capped sincos set (+-inf and the NaNs) come back with the other sign from the twin;
  * elu_det against exp_det - 1 and the IEEE operations against NumPy: the subtraction / division of the host and of the device each
    pass a NaN on by their own rule;
  * half -> float of the 1022 signalling binary16 NaNs: the hardware conversion quiets them, as IEEE 754 says a conversion does, the
    oracle's software conversion copies the payload — compared after setting the quiet bit in the oracle's result.
exp_det and log_det return a NaN argument itself through a select: every bit is compared, against the twins too.

One compile per session; each test is one or a few launches over at most a few million values.  A launch that ends in a HIP error makes
every later test of the module skip: a faulted card gets no more launches."""
import ctypes as C
import time

import numpy as np
import pytest

from env_build_amd import policy_sample as PS
from tests import _math_sets as S
from tests._math_sets import _fp, artanh_twin, bits_of as bits, oracle_fn
from tests._math_probe import DIVISORS, ProbeError, build_probe
from tests._helpers import oracle_lib

pytestmark = pytest.mark.gpu
F = S.F
_faulted = []                # the operations whose launch ended in a HIP error
_t0 = []


@pytest.fixture(scope='session')
def probe(tmp_path_factory):
    _t0.append(time.time())
    return build_probe(tmp_path_factory)


def run(probe, op, *args, **kw):
    if _faulted:
        pytest.skip('an earlier launch of the probe ended in a HIP error')
    try:
        return probe.run(op, *args, **kw)
    except ProbeError:
        _faulted.append(op)
        raise


def runf(probe, op, x, **kw):
    return run(probe, op, np.ascontiguousarray(x, F), **kw)


# ---- sin / cos ----
def test_sincos_equals_the_oracle_and_its_register_constant_form(probe):
    # what the device does from 2^31 * pi/2 on and at +-inf, said once in the output: the conversion saturates (v_cvt_i32_f32), so the
    # quadrant is that of INT_MAX (k & 3 == 3) above and of INT_MIN (k & 3 == 0) below; the oracle's cvt_i32_f32 states the same rule
    px = np.array([3e9, 4e9, 1e10, -1e10, np.inf, -np.inf], F)
    ps, pc = runf(probe, 'sincos', px)
    print('device sincos at 3e9, 4e9, 1e10, -1e10, inf, -inf: ' + ', '.join('(0x%08x, 0x%08x)' % t for t in zip(ps, pc)))
    x = S.full('sincos')
    s, c = runf(probe, 'sincos', x)
    ws, wc = oracle_fn('sincos', x)
    S.same_bits(s, ws, 'sin: device vs oracle', nan_bits=True)
    S.same_bits(c, wc, 'cos: device vs oracle', nan_bits=True)
    sk, ck = runf(probe, 'sincos_k', x)
    S.same_bits(sk, s, 'sin: sincos_det_k vs sincos_det', nan_bits=True)      # the same instructions on the same machine: NaNs too
    S.same_bits(ck, c, 'cos: sincos_det_k vs sincos_det', nan_bits=True)


def test_sincos_equals_the_numpy_twin(probe):
    x = S.capped('sincos')
    s, c = runf(probe, 'sincos', x)
    ws, wc = PS._sincos_det(x)
    S.same_bits(s, ws, 'sin: device vs NumPy twin')
    S.same_bits(c, wc, 'cos: device vs NumPy twin')


# ---- atan ----
def test_atan_equals_the_oracle(probe):
    x = S.full('atan')
    S.same_bits(runf(probe, 'atan', x), oracle_fn('atan', x), 'atan: device vs oracle', nan_bits=True)


# ---- exp / elu / tanh ----
def test_exp_equals_the_oracle_and_elu_is_exp_minus_one(probe):
    x = S.full('exp')
    e = runf(probe, 'exp', x)
    S.same_bits(e, oracle_fn('exp', x), 'exp: device vs oracle', nan_bits=True)
    elu = runf(probe, 'elu', x)
    with np.errstate(all='ignore'):
        want = np.where(x > 0, x, e.view(F) - F(1)).astype(F)                     # one IEEE subtraction on the host
    S.same_bits(elu, want, 'elu_det vs exp_det - 1 (x <= 0), x (x > 0)')
    pos = x > 0
    assert np.array_equal(elu[pos], bits(x)[pos])


def test_exp_and_tanh_equal_the_numpy_twins(probe):
    x = S.capped('exp')
    S.same_bits(runf(probe, 'exp', x), PS._exp_det(x), 'exp: device vs NumPy twin', nan_bits=True)
    x = S.capped('tanh')
    S.same_bits(runf(probe, 'tanh', x), PS._tanh_det(x), 'tanh: device vs NumPy twin')


def test_tanh_equals_the_oracle(probe):
    x = S.full('tanh')
    S.same_bits(runf(probe, 'tanh', x), oracle_fn('tanh', x), 'tanh: device vs oracle', nan_bits=True)


# ---- log / artanh: the NumPy twin is the only CPU text ----
def test_log_equals_the_numpy_twin(probe):
    x = S.capped('log')
    S.same_bits(runf(probe, 'log', x), PS._log_det(x), 'log: device vs NumPy twin', nan_bits=True)


def test_artanh_equals_the_numpy_twin(probe):
    u = S.capped('artanh')
    S.same_bits(runf(probe, 'artanh', u), artanh_twin(u), 'artanh: device vs NumPy twin')


# ---- the IEEE operations the contract takes for granted ----
@pytest.mark.parametrize('op', sorted(DIVISORS))
def test_div_const_and_div_by_are_ieee_division(probe, op):
    """v_cvt_f64_f32, v_mul_f64, v_cvt_f32_f64 on the device give x / c of IEEE fp32 division, subnormal quotients included (the
    exhaustive CPU check of tests/test_exact_math.py runs the same two operations on the host)"""
    x, c = S.common(), DIVISORS[op]
    with np.errstate(all='ignore'):
        want = x / F(c)
        S.same_bits(runf(probe, op, x), want, '%s: device vs IEEE x / c' % op)
        S.same_bits(runf(probe, 'div_by', x, rc=1.0 / c), want, 'div_by(x, 1 / %r)' % c)
        S.same_bits(runf(probe, 'div_by', x, rc=-1.0 / c), x / F(-c), 'div_by(x, -1 / %r)' % c)   # the sign rides on the reciprocal (turn_consts)


def test_deg2rad_and_rad2deg_are_the_two_ieee_operations(probe):
    x = S.common()
    with np.errstate(all='ignore'):
        S.same_bits(runf(probe, 'deg2rad', x), (x * F(np.pi)) / F(180), 'deg2rad')
        S.same_bits(runf(probe, 'rad2deg', x), (x * F(180)) / F(np.pi), 'rad2deg')


def test_division_reciprocal_and_square_root_are_correctly_rounded(probe):
    """`/` and __builtin_sqrtf as the product's flags compile them: IEEE bits, subnormal results included"""
    x, y = S.div_pairs()
    with np.errstate(all='ignore'):
        q = x / y
        S.same_bits(run(probe, 'div', x, y), q, 'x / y')
        assert (np.abs(q[np.isfinite(q)]) < F(2.0 ** -126)).sum() > 100000      # the set does reach subnormal quotients
        z = S.common()
        S.same_bits(runf(probe, 'rcp', z), F(1) / z, '1 / x')
        S.same_bits(runf(probe, 'sqrt', z), np.sqrt(z), 'sqrtf')


# ---- binary16 storage ----
def test_half_conversions_equal_the_oracle(probe):
    lib = oracle_lib().lib
    x = S.f16_set()
    back, hb = runf(probe, 'f32_to_f16', x)
    want = np.empty(x.size, np.uint16)
    lib.eb_oracle_float_to_half(_fp(x), _fp(want), x.size)
    nan = np.isnan(x)
    print('float -> half: %d of %d NaN arguments encoded differently from the oracle' % ((hb[nan] != want[nan]).sum(), nan.sum()))
    assert np.array_equal(hb, want.astype(np.uint32)), 'float -> half'                                                # NaNs included
    wide = np.empty(x.size, F)
    h16 = np.ascontiguousarray(hb.astype(np.uint16))
    lib.eb_oracle_half_to_float(_fp(h16), _fp(wide), x.size)
    S.same_bits(back, wide, 'float -> half -> float')
    allh = np.arange(1 << 16, dtype=np.uint32)                                                                        # all 65 536 halves
    f = np.empty(allh.size, F)
    a16 = np.ascontiguousarray(allh.astype(np.uint16))
    lib.eb_oracle_half_to_float(_fp(a16), _fp(f), allh.size)
    fb = bits(f).copy()
    fb[np.isnan(f)] |= np.uint32(0x00400000)                                                                          # a signalling NaN comes out quiet
    assert (fb != bits(f)).sum() == 1022
    S.same_bits(run(probe, 'f16_to_f32', allh), fb, 'half -> float', nan_bits=True)


# ---- the counter-based noise ----
def test_u01_equals_the_numpy_twin(probe):
    rng = np.random.default_rng(7)
    key = rng.integers(0, 1 << 64, 200000, dtype=np.uint64)
    idx = rng.integers(0, 1 << 64, 200000, dtype=np.uint64)
    idx[:1000] = np.arange(1000, dtype=np.uint64)
    ek = [(k, i) for k, _ in S.extreme_keys() for i in (0, 1)]
    key = np.concatenate([key, np.array([k for k, _ in ek], np.uint64)])
    idx = np.concatenate([idx, np.array([i for _, i in ek], np.uint64)])
    with np.errstate(over='ignore'):
        want = PS._u01(key, idx)
    got = run(probe, 'u01', key, idx)
    S.same_bits(got, want, 'u01', nan_bits=True)
    assert got.view(F).min() == 0 and got.view(F).max() == F(1) - F(2.0 ** -24)      # the constructed keys reach both ends of [0, 1)


def _device_noise(probe, row_ids, act_dim, seed, counter):
    """policy_noise_reference's arguments -> the same [n, act_dim] array from normal_pair on the device"""
    P = (act_dim + 1) // 2
    key = S.splitmix64((int(seed) + S.GOLDEN * int(counter)) & S.M64)
    ids = np.repeat(np.asarray(row_ids, np.uint64), P)
    p = np.tile(np.arange(P, dtype=np.int32), len(row_ids))
    e0, e1 = run(probe, 'normal', np.full(ids.size, key, np.uint64), ids, p, P=P)
    eps = np.empty((len(row_ids), 2 * P), np.uint32)
    eps[:, 0::2], eps[:, 1::2] = e0.reshape(-1, P), e1.reshape(-1, P)
    return np.ascontiguousarray(eps[:, :act_dim])


def test_normal_pair_equals_the_noise_reference(probe):
    rows = np.concatenate([np.arange(20000), [2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]]).astype(np.uint64)
    for act_dim, seed, counter in ((5, 1234567, 89), (2, 2 ** 64 - 1, 2 ** 63 + 5)):
        got = _device_noise(probe, rows, act_dim, seed, counter)
        S.same_bits(got, PS.policy_noise_reference(rows, act_dim, seed, counter), 'normal_pair, act_dim %d' % act_dim, nan_bits=True)


def test_normal_pair_at_the_constructed_extremes(probe):
    """u = 1 (radius 0), u = 2^-24 (the largest radius), v = 0 and v = 1 - 2^-24, alone and together: finite, and the reference's bits"""
    for key, what in S.extreme_keys():
        seed = S.seed_of_key(key)
        got = _device_noise(probe, np.array([0], np.uint64), 2, seed, 0)
        assert np.isfinite(got.view(F)).all(), what
        S.same_bits(got, PS.policy_noise_reference([0], 2, seed, 0), 'normal_pair: ' + what, nan_bits=True)
    big = _device_noise(probe, np.array([0], np.uint64), 2, S.seed_of_key(S.JOINT_KEYS[1][0]), 0).view(F)
    assert 5.76 < big[0, 0] < 5.77 and big[0, 1] == 0                             # sqrt(-2 log 2^-24) = 5.768 on the cosine side


def test_zz_wall_time_of_the_module(probe):
    print('math probe module: %.1f s from the compile to here; faulted launches: %s' % (time.time() - _t0[0], _faulted))
