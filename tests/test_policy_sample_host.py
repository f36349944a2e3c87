"""CPU (-m "not gpu"): the stochastic policy head (include/envbuild_policy_sample.h, env_build_amd.policy_sample) — its header against
the module's own binding table, the built library's exports and device-free refusals, the NumPy restatement of the contract against
torch.distributions and torch autograd in float64 and against itself in float32, the deterministic logarithm's error and the
counter-based noise's statistics."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import policy_sample as ps
from tests._helpers import ROOT, oracle_lib

HEADER = os.path.join(ROOT, 'include', 'envbuild_policy_sample.h')
KERNELS = ('policy_sample_kernel', 'policy_sample_logits_kernel', 'policy_sample_vjp_kernel')


def test_header_declares_what_the_module_binds():
    text = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(ps.POLICY_SAMPLE_PROTOTYPES) == sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert sorted(ps.POLICY_SAMPLE_PROTOTYPES) == ['eb_policy_sample', 'eb_policy_sample_abi_version', 'eb_policy_sample_from_logits',
                                                   'eb_policy_sample_supported', 'eb_policy_sample_vjp']
    for name, (_res, args) in ps.POLICY_SAMPLE_PROTOTYPES.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, name
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert {n: len(a) for n, (_r, a) in ps.POLICY_SAMPLE_PROTOTYPES.items()} == {
        'eb_policy_sample_abi_version': 0, 'eb_policy_sample_supported': 2, 'eb_policy_sample': 13, 'eb_policy_sample_from_logits': 12,
        'eb_policy_sample_vjp': 9}
    assert int(re.search(r'#define EB_POLICY_SAMPLE_ABI_VERSION (\d+)', text).group(1)) == ps.EB_POLICY_SAMPLE_ABI_VERSION == 1
    for words in ('bit for bit', 'log_det', 'splitmix64', 'eb_mlp_backward(head = 0)', 'ALWAYS exactly one launch', 'policy_sample_reference',
                  '0.9189385332f', '6.2831855f'):
        assert words in text, words


def test_the_family_tables_are_untouched():
    assert list(_capi.FAMILIES) == ['grad', 'cand', 'cand_grad', 'sample', 'ilqr', 'mlp_f16', 'policy_rollout', 'mlp_grad',
                                    'policy_rollout_grad']
    assert not set(ps.POLICY_SAMPLE_PROTOTYPES) & set(_capi.PROTOTYPES)
    for row in _capi.FAMILIES.values():
        assert not set(ps.POLICY_SAMPLE_PROTOTYPES) & set(row[5])
    assert 'eb_policy_sample' not in open(os.path.join(ROOT, 'include', 'envbuild.h')).read()


@pytest.fixture(scope='module')
def hip_library():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    lib.eb_last_error.restype = C.c_char_p
    for name, (res, args) in ps.POLICY_SAMPLE_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, open(lib_path, 'rb').read()


def test_the_library_exports_the_entries_and_the_kernels(hip_library):
    lib, blob = hip_library
    assert lib.eb_policy_sample_abi_version() == 1
    assert b'gfx950' in blob
    for kernel in KERNELS:
        assert kernel.encode() in blob, kernel
    public = os.path.join('..', '..', 'include', 'envbuild_policy_sample.h')
    assert 'eb_policy_sample.hip' in eb_build.SOURCES
    assert {'eb_policy_sample.h', 'eb_policy_sample_device.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not [f for f in files if 'policy_sample' in f]


def test_refusals_need_no_device_and_name_their_entry(hip_library):
    lib, _ = hip_library
    seven = C.c_int32(7)
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    calls = [
        ('eb_policy_sample_supported', (None, C.byref(seven))),
        ('eb_policy_sample', (None, 4, p, None, None, 0, 0, 1.0, p, None, None, None, None)),
        ('eb_policy_sample_from_logits', (4, 2, None, None, None, 0, 0, 1.0, p, None, None, None)),      # NULL logits
        ('eb_policy_sample_from_logits', (4, 2, p, None, None, 0, 0, 1.0, None, None, None, None)),      # NULL actions
        ('eb_policy_sample_from_logits', (1, 3, p, None, None, 0, 0, 1.0, p, None, None, None)),         # odd out_dim
        ('eb_policy_sample_from_logits', (1, 34, p, None, None, 0, 0, 1.0, p, None, None, None)),        # out_dim > 32
        ('eb_policy_sample_from_logits', (1, 2, p, None, None, 0, 0, float('nan'), p, None, None, None)),
        ('eb_policy_sample_from_logits', (-1, 2, p, None, None, 0, 0, 1.0, p, None, None, None)),
        ('eb_policy_sample_vjp', (4, 2, None, p, 1.0, None, None, p, None)),
        ('eb_policy_sample_vjp', (4, 2, p, None, 1.0, None, None, p, None)),
        ('eb_policy_sample_vjp', (4, 2, p, p, 1.0, None, None, None, None)),
        ('eb_policy_sample_vjp', (1, 5, p, p, 1.0, None, None, p, None)),
        ('eb_policy_sample_vjp', (1, 34, p, p, 1.0, None, None, p, None)),
        ('eb_policy_sample_vjp', (1, 2, p, p, float('nan'), None, None, p, None)),
    ]
    for name, args in calls:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert lib.eb_last_error().startswith(name.encode() + b':'), (name, lib.eb_last_error())
    assert seven.value == 7 and all(v == 0.0 for v in buf)
    # n = 0 is a no-op that needs no pointer and no device
    assert lib.eb_policy_sample_from_logits(0, 2, None, None, None, 0, 0, 1.0, None, None, None, None) == 0
    assert lib.eb_policy_sample_vjp(0, 2, None, None, 1.0, None, None, None, None) == 0


def test_a_library_without_the_entries_is_refused_by_header_name():
    api = oracle_lib()
    assert api.backend == 'oracle'
    with pytest.raises(_capi.EbError) as e:
        ps.bind(api)
    assert 'envbuild_policy_sample.h' in str(e.value) and 'eb_policy_sample_from_logits' in str(e.value)


# ---- the restatement against torch.distributions and autograd --------------------------------------------------------------------------
def case(act_dim, n=24, seed=0):
    rng = np.random.default_rng(1000 * act_dim + seed)
    mean = (1.5 * rng.standard_normal((n, act_dim))).astype(np.float32)
    ls = rng.uniform(-4.0, 1.0, (n, act_dim)).astype(np.float32)
    eps = rng.standard_normal((n, act_dim)).astype(np.float32)
    g_a = rng.standard_normal((n, act_dim)).astype(np.float32)
    g_lp = rng.standard_normal(n).astype(np.float32)
    return np.concatenate([mean, ls], axis=1), eps, g_a, g_lp


def torch_yardstick(logits, eps, action_range, g_a, g_lp):
    """float64: TransformedDistribution(Independent(Normal), [TanhTransform, AffineTransform]).log_prob of the reparameterised sample, and
    autograd of sum(g_a * actions) + sum(g_lp * logp) with respect to the logits"""
    import torch
    from torch import distributions as D
    y = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(eps, np.float64))
    act_dim = y.shape[1] // 2
    mean, ls = y[:, :act_dim], y[:, act_dim:]
    base = D.Independent(D.Normal(mean, ls.exp()), 1)
    x = mean + ls.exp() * e
    if action_range is None:
        actions, logp = x, base.log_prob(x)
    else:
        tanh = D.transforms.TanhTransform(cache_size=1)
        dist = D.TransformedDistribution(base, [tanh, D.transforms.AffineTransform(0.0, float(action_range), cache_size=1)])
        t = tanh(x)
        actions = dist.transforms[1](t)
        logp = dist.log_prob(actions)
    ((actions * torch.tensor(np.asarray(g_a, np.float64))).sum() + (logp * torch.tensor(np.asarray(g_lp, np.float64))).sum()).backward()
    return actions.detach().numpy(), logp.detach().numpy(), y.grad.numpy()


def within(got, want, bar, what):
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, np.float64) - want).max()
    assert err <= bar * scale, '%s: error %.3g of a maximum of %.3g (bar %.1g)' % (what, err, scale, bar)


@pytest.mark.parametrize('action_range', [1.0, 0.5, None])
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float64_restatement_equals_torch_distributions_and_autograd(act_dim, action_range):
    logits, eps, g_a, g_lp = case(act_dim)
    want = torch_yardstick(logits, eps, action_range, g_a, g_lp)
    got = ps.policy_sample_reference(logits, eps, action_range, g_a, g_lp, dtype=np.float64)
    for name, g, w in zip(('actions', 'logp', 'g_logits'), got, want):
        within(g, w, 1e-12, '%s, act_dim %d, action_range %r' % (name, act_dim, action_range))
    # each cotangent alone: None means zeros
    zeros_a, zeros_lp = np.zeros_like(g_a), np.zeros_like(g_lp)
    only_lp = ps.policy_sample_reference(logits, eps, action_range, None, g_lp, dtype=np.float64)[2]
    only_a = ps.policy_sample_reference(logits, eps, action_range, g_a, None, dtype=np.float64)[2]
    within(only_lp, torch_yardstick(logits, eps, action_range, zeros_a, g_lp)[2], 1e-12, 'g_logp alone')
    within(only_a, torch_yardstick(logits, eps, action_range, g_a, zeros_lp)[2], 1e-12, 'g_actions alone')
    assert ps.policy_sample_reference(logits, eps, action_range, dtype=np.float64)[2] is None


@pytest.mark.parametrize('action_range', [1.0, 0.5, None])
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float32_restatement_is_within_the_project_bar_of_float64(act_dim, action_range):
    logits, eps, g_a, g_lp = case(act_dim)
    want = ps.policy_sample_reference(logits, eps, action_range, g_a, g_lp, dtype=np.float64)
    got = ps.policy_sample_reference(logits, eps, action_range, g_a, g_lp, dtype=np.float32)
    for name, g, w in zip(('actions', 'logp', 'g_logits'), got, want):
        assert g.dtype == np.float32
        within(g, w, 1e-5, '%s, act_dim %d, action_range %r' % (name, act_dim, action_range))


def test_fmaf_rounds_once():
    # (1 + 2^-12)^2 is 1 + 2^-11 + 2^-24: minus (1 + 2^-11) the fused result is the product's last bit, 2^-24
    a = np.float32(1 + 2.0 ** -12)
    assert ps._fmaf(a, a, np.float32(-(1 + 2.0 ** -11)))[()] == np.float32(2.0 ** -24)
    # a double-rounding witness: (1 + 3 * 2^-23) * 1.5 = 1.5 + 4 * 2^-23 + 2^-24 is a float32 tie; + 2^-54 lies just above it, so one
    # rounding goes up to 1.5 + 5 * 2^-23; float64 rounds the sum onto the tie first and the second rounding goes to even, 1.5 + 4 * 2^-23
    x, y, z = np.float32(1 + 3 * 2.0 ** -23), np.float32(1.5), np.float32(2.0 ** -54)
    assert ps._fmaf(x, y, z)[()] == np.float32(1.5 + 5 * 2.0 ** -23)
    from env_build_amd.policy import _fma32
    assert _fma32(x, y, z)[()] == np.float32(1.5 + 4 * 2.0 ** -23)


LOG_DET_WORST_ULPS = 0.7902     # measured on the CPU over the two sweeps below (0.7902 on (0, 2], 0.7454 on the log-spaced one)


def test_log_det_against_float64():
    worst = 0.0
    for x in (np.linspace(0.0, 2.0, 200001)[1:].astype(np.float32), np.logspace(-30.0, 30.0, 100001).astype(np.float32)):
        want = np.log(x.astype(np.float64))
        ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
        ulp = np.maximum(ulp, float(np.finfo(np.float32).tiny) * 2.0 ** -23)
        err = np.abs(ps._log_det(x).astype(np.float64) - want) / ulp
        worst = max(worst, float(err.max()))
    print('log_det: worst error %.4f ulp' % worst)
    assert worst <= LOG_DET_WORST_ULPS + 1.0
    assert ps._log_det(np.array([1.0], np.float32))[0] == 0.0
    assert np.isnan(ps._log_det(np.array([np.nan], np.float32))[0])


# measured on the CPU for 65 536 rows x 2 under (seed 0, counter 0); a library generator at this size gave KS 0.0013, variance 0.997
NOISE_MEAN, NOISE_VAR_OFF, NOISE_KS = 1.0196e-3, 3.8083e-3, 1.9151e-3


@pytest.fixture(scope='module')
def noise():
    return ps.policy_noise_reference(np.arange(65536), 2, 0, 0)


def test_noise_restatement_is_standard_normal(noise):
    assert noise.shape == (65536, 2) and noise.dtype == np.float32
    z = np.sort(noise.ravel().astype(np.float64))
    n = len(z)
    cdf = 0.5 * (1.0 + np.array([math.erf(v / math.sqrt(2.0)) for v in z]))
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(0, n) / n))
    print('noise: mean %.4e, variance %.6f, KS %.4e, largest |eps| %.3f' % (z.mean(), z.var(), ks, np.abs(z).max()))
    assert abs(z.mean()) <= 2 * NOISE_MEAN
    assert abs(z.var() - 1.0) <= 2 * NOISE_VAR_OFF
    assert ks <= 2 * NOISE_KS
    assert np.abs(z).max() <= 5.77


def test_noise_depends_on_the_row_id_and_the_pair_only(noise):
    ids = np.arange(512)
    base = noise[:512]
    assert not np.array_equal(ps.policy_noise_reference(ids, 2, 1, 0), base)
    assert not np.array_equal(ps.policy_noise_reference(ids, 2, 0, 1), base)
    assert not np.array_equal(ps.policy_noise_reference(ids, 2, 1, 0), ps.policy_noise_reference(ids, 2, 0, 1))
    perm = np.random.default_rng(3).permutation(512)
    assert np.array_equal(ps.policy_noise_reference(perm, 2, 0, 0), base[perm])
    assert np.array_equal(ps.policy_noise_reference(ids, 2, 0, 0), base)
    # an odd act_dim drops the last pair's second draw: P = 2 pairs per row
    three = ps.policy_noise_reference(ids, 3, 0, 0)
    four = ps.policy_noise_reference(ids, 4, 0, 0)
    assert three.shape == (512, 3) and np.array_equal(three, four[:, :3])
    # ids are unsigned 32-bit numbers
    assert np.array_equal(ps.policy_noise_reference(np.array([-1], np.int32), 2, 0, 0), ps.policy_noise_reference(np.array([2 ** 32 - 1]), 2, 0, 0))
