"""CPU (-m "not gpu"): the log-probability of given actions (include/envbuild_policy_logp.h, env_build_amd.policy_logp) — its header
against the module's own binding table, the built library's exports and device-free refusals, the NumPy restatement of the contract
against torch.distributions and torch autograd in float64 and against itself in float32, the round trip through the sampler's
restatement, and the clamp at +-action_range."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from tests._helpers import ROOT, oracle_lib

HEADER = os.path.join(ROOT, 'include', 'envbuild_policy_logp.h')
KERNELS = ('policy_logp_kernel', 'policy_logp_logits_kernel', 'policy_logp_vjp_kernel')
RANGES = (1.0, 0.5, None)


def test_header_declares_what_the_module_binds():
    text = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(pl.POLICY_LOGP_PROTOTYPES) == sorted(set(re.findall(r'\b(eb_policy_[a-z0-9_]+)\s*\(', src)))
    assert sorted(pl.POLICY_LOGP_PROTOTYPES) == ['eb_policy_logp', 'eb_policy_logp_abi_version', 'eb_policy_logp_from_logits',
                                                 'eb_policy_logp_supported', 'eb_policy_logp_vjp']
    for name, (_res, args) in pl.POLICY_LOGP_PROTOTYPES.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, name
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert {n: len(a) for n, (_r, a) in pl.POLICY_LOGP_PROTOTYPES.items()} == {
        'eb_policy_logp_abi_version': 0, 'eb_policy_logp_supported': 2, 'eb_policy_logp': 2, 'eb_policy_logp_from_logits': 1,
        'eb_policy_logp_vjp': 1}
    assert int(re.search(r'#define EB_POLICY_LOGP_ABI_VERSION (\d+)', text).group(1)) == pl.EB_POLICY_LOGP_ABI_VERSION == 1
    # no entry takes a stream parameter: the stream is a field of the struct
    assert not re.search(r'\bint\s+eb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)
    # the struct's fields, in the header's order, are the binding's
    body = re.search(r'typedef struct eb_policy_logp_args \{(.*?)\} eb_policy_logp_args;', src, flags=re.S).group(1)
    fields = [re.search(r'(\w+)$', part.strip()).group(1) for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert fields == [name for name, _ in pl.EbPolicyLogpArgs._fields_]
    for words in ('bit for bit', 'log_det', 'eb_mlp_backward(head = 0)', 'ALWAYS exactly one launch', 'policy_logp_reference',
                  '0.9189385332f', '0.6931471806f', '0x1.fffffep-1f', '8.664', 'AT CALL TIME', 'tests/test_stream_census.py',
                  '1.6e-4', 'IEEE division'):
        assert words in text, words


def test_the_family_tables_are_untouched():
    assert not set(pl.POLICY_LOGP_PROTOTYPES) & set(_capi.PROTOTYPES)
    for row in _capi.FAMILIES.values():
        assert not set(pl.POLICY_LOGP_PROTOTYPES) & set(row[5])
    assert not set(pl.POLICY_LOGP_PROTOTYPES) & set(ps.POLICY_SAMPLE_PROTOTYPES)
    for header in ('envbuild.h', 'envbuild_policy_sample.h'):
        assert 'eb_policy_logp' not in open(os.path.join(ROOT, 'include', header)).read()


@pytest.fixture(scope='module')
def hip_library():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    lib.eb_last_error.restype = C.c_char_p
    for name, (res, args) in pl.POLICY_LOGP_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, open(lib_path, 'rb').read()


def test_the_library_exports_the_entries_and_the_kernels(hip_library):
    lib, blob = hip_library
    assert lib.eb_policy_logp_abi_version() == 1
    assert b'gfx950' in blob
    for kernel in KERNELS:
        assert kernel.encode() in blob, kernel
    public = os.path.join('..', '..', 'include', 'envbuild_policy_logp.h')
    assert 'eb_policy_logp.hip' in eb_build.SOURCES
    assert {'eb_policy_logp.h', 'eb_policy_logp_device.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not [f for f in files if 'policy_logp' in f]
    # every header the translation unit includes is hashed with it
    unit = open(os.path.join(eb_build.CSRC, 'eb_policy_logp.hip')).read()
    assert set(re.findall(r'#include "(eb_[a-z0-9_]+\.h)"', unit)) <= set(eb_build.HEADERS)


def test_refusals_need_no_device_and_name_their_entry(hip_library):
    lib, _ = hip_library
    seven = C.c_int32(7)
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    nan = float('nan')

    def args(n=4, out_dim=2, action_range=1.0, **kw):
        full = dict(obs=p, logits=p, actions=p, logp=p, z=p, g_logp=p, g_logits=p)
        full.update(kw)
        return C.byref(pl.EbPolicyLogpArgs(n=n, out_dim=out_dim, action_range=action_range, **full))

    calls = [
        ('eb_policy_logp_supported', (None, C.byref(seven))),
        ('eb_policy_logp', (None, args())),
        ('eb_policy_logp', (None, None)),
        ('eb_policy_logp_from_logits', (None,)),
        ('eb_policy_logp_from_logits', (args(logits=None),)),
        ('eb_policy_logp_from_logits', (args(actions=None),)),
        ('eb_policy_logp_from_logits', (args(logp=None),)),
        ('eb_policy_logp_from_logits', (args(n=1, out_dim=3),)),
        ('eb_policy_logp_from_logits', (args(n=1, out_dim=34),)),
        ('eb_policy_logp_from_logits', (args(n=1, out_dim=0),)),
        ('eb_policy_logp_from_logits', (args(n=1, action_range=nan),)),
        ('eb_policy_logp_from_logits', (args(n=-1),)),
        ('eb_policy_logp_vjp', (None,)),
        ('eb_policy_logp_vjp', (args(logits=None),)),
        ('eb_policy_logp_vjp', (args(z=None),)),
        ('eb_policy_logp_vjp', (args(g_logp=None),)),
        ('eb_policy_logp_vjp', (args(g_logits=None),)),
        ('eb_policy_logp_vjp', (args(n=1, out_dim=5),)),
        ('eb_policy_logp_vjp', (args(n=1, out_dim=34),)),
        ('eb_policy_logp_vjp', (args(n=-1),)),
    ]
    for name, a in calls:
        assert getattr(lib, name)(*a) == -1, name
        assert lib.eb_last_error().startswith(name.encode() + b':'), (name, lib.eb_last_error())
    assert seven.value == 7 and all(v == 0.0 for v in buf)
    # n = 0 is a no-op that needs no pointer and no device
    empty = pl.EbPolicyLogpArgs(n=0, out_dim=2, action_range=1.0)
    assert lib.eb_policy_logp_from_logits(C.byref(empty)) == 0
    assert lib.eb_policy_logp_vjp(C.byref(empty)) == 0


def test_a_library_without_the_entries_is_refused_by_header_name():
    api = oracle_lib()
    assert api.backend == 'oracle'
    with pytest.raises(_capi.EbError) as e:
        pl.bind(api)
    assert 'envbuild_policy_logp.h' in str(e.value) and 'eb_policy_logp_from_logits' in str(e.value)


# ---- the restatement against torch.distributions and autograd --------------------------------------------------------------------------
def case(act_dim, n=24, seed=0):
    """logits (mean 0.5 N(0, 1), log_std uniform in [-2, 1]), the noise, and a cotangent of logp"""
    rng = np.random.default_rng(1000 * act_dim + seed)
    mean = (0.5 * rng.standard_normal((n, act_dim))).astype(np.float32)
    ls = rng.uniform(-2.0, 1.0, (n, act_dim)).astype(np.float32)
    eps = rng.standard_normal((n, act_dim)).astype(np.float32)
    g_lp = rng.standard_normal(n).astype(np.float32)
    return np.concatenate([mean, ls], axis=1), eps, g_lp


def sampled(act_dim, action_range, dtype=np.float32):
    """the case with actions from the sampler's restatement under that noise"""
    logits, eps, g_lp = case(act_dim)
    actions = ps.policy_sample_reference(logits, eps, action_range, dtype=dtype)[0]
    return logits, eps, actions, g_lp


def torch_yardstick(logits, actions, action_range, g_lp):
    """float64: TransformedDistribution(Independent(Normal), [TanhTransform, AffineTransform]).log_prob(actions), and autograd of
    sum(g_lp * logp) with respect to the logits"""
    import torch
    from torch import distributions as D
    y = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    a = torch.tensor(np.asarray(actions, np.float64))
    act_dim = y.shape[1] // 2
    mean, ls = y[:, :act_dim], y[:, act_dim:]
    dist = D.Independent(D.Normal(mean, ls.exp()), 1)
    if action_range is not None:
        dist = D.TransformedDistribution(dist, [D.transforms.TanhTransform(), D.transforms.AffineTransform(0.0, float(action_range))])
    logp = dist.log_prob(a)
    (logp * torch.tensor(np.asarray(g_lp, np.float64))).sum().backward()
    return logp.detach().numpy(), y.grad.numpy()


def within(got, want, bar, what):
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want).max()
    print('%s: error %.3g of a maximum of %.3g' % (what, err, scale))
    assert err <= bar * scale, '%s: error %.3g of a maximum of %.3g (bar %.1g)' % (what, err, scale, bar)


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float64_restatement_equals_torch_distributions_and_autograd(act_dim, action_range):
    logits, _, actions, g_lp = sampled(act_dim, action_range)
    want = torch_yardstick(logits, actions, action_range, g_lp)
    logp, z, g_logits = pl.policy_logp_reference(logits, actions, action_range, g_lp, dtype=np.float64)
    assert logp.dtype == z.dtype == g_logits.dtype == np.float64
    within(logp, want[0], 1e-12, 'logp, act_dim %d, action_range %r' % (act_dim, action_range))
    within(g_logits, want[1], 1e-12, 'g_logits, act_dim %d, action_range %r' % (act_dim, action_range))
    assert pl.policy_logp_reference(logits, actions, action_range, dtype=np.float64)[2] is None


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float32_restatement_is_within_the_project_bar_of_float64(act_dim, action_range):
    logits, _, actions, g_lp = sampled(act_dim, action_range)
    want = pl.policy_logp_reference(logits, actions, action_range, g_lp, dtype=np.float64)
    got = pl.policy_logp_reference(logits, actions, action_range, g_lp, dtype=np.float32)
    for name, g, w in zip(('logp', 'z', 'g_logits'), got, want):
        assert g.dtype == np.float32
        within(g, w, 1e-5, '%s, act_dim %d, action_range %r' % (name, act_dim, action_range))


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float64_round_trip_recovers_the_noise_and_the_samplers_logp(act_dim, action_range):
    """With float64 actions z is the noise and logp the sampler's formula, to 1e-8 absolute: the rounding of u is amplified by
    1 / ((1 - u^2) std), which stays below about 1e-10 while |x| <= 6 and std >= e^-2.  That is a condition on the inputs: asserted."""
    logits, eps, g_lp = case(act_dim)
    y, e = logits.astype(np.float64), eps.astype(np.float64)
    x = y[:, :act_dim] + np.exp(y[:, act_dim:]) * e
    assert np.abs(x).max() <= 6.0 and y[:, act_dim:].min() >= -2.0
    actions, want_logp, _ = ps.policy_sample_reference(logits, eps, action_range, dtype=np.float64)
    assert actions.dtype == np.float64
    logp, z, _ = pl.policy_logp_reference(logits, actions, action_range, dtype=np.float64)
    err_z, err_lp = np.abs(z - e).max(), np.abs(logp - want_logp).max()
    print('round trip: |z - eps| %.3g, |logp - sampler| %.3g, largest |x| %.3g' % (err_z, err_lp, np.abs(x).max()))
    assert err_z <= 1e-8 and err_lp <= 1e-8


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_clamp_makes_actions_at_and_beyond_the_range_finite(dtype):
    ar = 0.5
    x_max = math.atanh(1.0 - 2.0 ** -24)                           # 8.664
    assert abs(x_max - 8.664) < 1e-3
    logits = np.array([[0.25, -0.5]] * 8, np.float32)              # mean, log_std
    actions = np.array([[ar], [-ar], [2 * ar], [-3 * ar], [np.inf], [-np.inf], [np.nan], [0.1]], np.float32)
    logp, z, g = pl.policy_logp_reference(logits, actions, ar, np.ones(8, np.float32), dtype=dtype)
    x = z.astype(np.float64) * math.exp(-0.5) + 0.25               # undo the standardisation
    sign = np.array([1, -1, 1, -1, 1, -1], np.float64)
    assert np.allclose(x[:6, 0], sign * x_max, rtol=0, atol=1e-5 if dtype == np.float32 else 1e-12)
    assert np.isfinite(logp[:6]).all() and np.isfinite(g[:6]).all()
    # both signs of the same magnitude: one clamp
    assert logp[0] == logp[2] == logp[4] and logp[1] == logp[3] == logp[5]
    # a NaN action gives a NaN row and leaves its neighbours alone
    assert np.isnan(logp[6]) and np.isnan(z[6]).all() and np.isnan(g[6]).all()
    assert np.isfinite(logp[7]) and np.isfinite(z[7]).all() and np.isfinite(g[7]).all()
    # without a range nothing is clamped
    free = pl.policy_logp_reference(logits, actions, None, dtype=dtype)
    assert np.array_equal(free[1][:4, 0].astype(np.float64) * math.exp(-0.5) + 0.25 > 0, [True, False, True, False])
    assert not np.isfinite(free[0][4]) and np.isnan(free[0][6])
