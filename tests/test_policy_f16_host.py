"""CPU (-m "not gpu"): the fp16 policy family (include/envbuild_mlp_f16.h) is declared as ctypes binds it, lives in a family table of
its own next to the five of _capi.FAMILIES, is exported by the built library next to a gfx950 mlp_f16_kernel, stays out of the hashed
forward sources and is refused by name by the oracle library; and the NumPy restatement of its contract
(env_build_amd.policy.mlp_f16_reference) holds the GPU test's bound under a second accumulation order and reproduces the reference's
safe flags on the G14 fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd.policy import _tanh_det, mlp_f16_reference
from tests._grad_cases import column_tolerance
from tests._helpers import ROOT, HostModel, golden, oracle_lib
from tests._policy_cases import G14, make_layers

HEADER = 'envbuild_mlp_f16.h'
# tests/test_gpu_policy.py's CONFIGS (that module is GPU-marked as a whole; restated here) plus the smallest network
CONFIGS = [
    (41, 2, 256, 4, 'elu', 'linear'), (137, 2, 256, 4, 'elu', 'linear'), (29, 1, 64, 4, 'relu', 'linear'),
    (45, 3, 128, 1, 'tanh', 'relu'), (265, 2, 512, 4, 'elu', 'tanh'), (33, 4, 100, 6, 'elu', 'linear'),
    (8, 8, 32, 2, 'elu', 'linear'), (137, 2, 300, 32, 'relu', 'linear'), (300, 1, 256, 4, 'elu', 'linear'),
    (17, 1, 1, 1, 'elu', 'linear'),
]


def header_src():
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_declares_what_ctypes_binds():
    text, src = header_src()
    protos = _capi.MLP_F16_PROTOTYPES
    assert sorted(protos) == sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    for name, (_res, args) in protos.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/%s' % (name, HEADER)
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert not set(protos) & set(_capi.PROTOTYPES)
    for row in _capi.FAMILIES.values():
        assert not set(protos) & set(row[5])
    for words in ('round-to-nearest-even', 'subnormal', 'NOT part of the contract', 'mlp_f16_reference'):
        assert words in text, words


def test_abi_numbers_and_the_second_family_table():
    _text, src = header_src()
    assert int(re.search(r'#define EB_MLP_F16_ABI_VERSION (\d+)', src).group(1)) == _capi.EB_MLP_F16_ABI_VERSION == 1
    for name, value in (('EB_MLP_PRECISION_F32', 0), ('EB_MLP_PRECISION_F16', 1)):
        assert int(re.search(r'#define %s (\d+)' % name, src).group(1)) == value
    assert _capi.MLP_PRECISION_ID == {'fp32': 0, 'fp16': 1}
    assert list(_capi.FAMILIES) == ['grad', 'cand', 'cand_grad', 'sample', 'ilqr']
    assert list(_capi.MORE_FAMILIES) == ['mlp_f16']
    row = _capi.MORE_FAMILIES['mlp_f16']
    assert len(row) == 6 == len(_capi.FAMILIES['grad'])
    assert row[0] == HEADER and row[3] == 'eb_mlp_f16_abi_version' and row[4] == 1 and row[5] is _capi.MLP_F16_PROTOTYPES
    assert _capi.family_row('mlp_f16') is row and _capi.family_row('grad') is _capi.FAMILIES['grad']


def test_hip_library_exports_the_entries_and_a_gfx950_kernel():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib, blob = C.CDLL(lib_path), open(lib_path, 'rb').read()
    for name in _capi.MLP_F16_PROTOTYPES:
        assert hasattr(lib, name), name
    assert lib.eb_mlp_f16_abi_version() == 1
    assert b'gfx950' in blob and b'mlp_f16_kernel' in blob
    public = os.path.join('..', '..', 'include', HEADER)
    assert 'eb_policy_f16.hip' in eb_build.SOURCES and {'eb_policy_f16.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not set(files) & {'eb_policy_f16.hip', 'eb_policy_f16.h', public}
    # the refusals need no device: the handle is checked first
    p = C.c_int32(7)
    assert lib.eb_mlp_set_precision(None, 1) == -1 and lib.eb_mlp_get_precision(None, C.byref(p)) == -1 and p.value == 7
    lib.eb_last_error.restype = C.c_char_p
    assert b'eb_mlp_get_precision' in lib.eb_last_error()


def test_the_oracle_library_is_refused_with_the_family_label_and_header():
    api = oracle_lib()
    assert api.backend == 'oracle'
    header, label = _capi.MORE_FAMILIES['mlp_f16'][:2]
    for name in ('mlp_set_precision', 'mlp_get_precision', 'mlp_f16_abi_version'):
        assert 'eb_' + name in _capi.MLP_F16_PROTOTYPES
        with pytest.raises(_capi.EbError) as e:
            getattr(api, name)
        assert label in str(e.value) and header in str(e.value), name
        for fn in (api.mlp_f16_fn, lambda s: api.family_fn('mlp_f16', s)):
            with pytest.raises(_capi.EbError) as e:
                fn('eb_' + name)
            assert label in str(e.value) and header in str(e.value), name
    assert api.family_fn.__doc__ and not hasattr(api.lib, 'eb_mlp_set_precision')


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '%dx%dx%d_%s' % (c[0], c[1], c[2], c[4]))
def test_restatement_holds_the_bound_under_a_second_accumulation_order(cfg):
    """the GPU test's bound (tests/test_gpu_policy_f16.py, test 2) with another order standing in for the kernel's: blocks of 16 k summed
    exactly, rounded once per block, the blocks taken in reverse.  Measured worst error / tolerance over the ten configs: 0.45."""
    obs_dim, n_hidden, n_units, out_dim, hact, oact = cfg
    rng = np.random.default_rng(obs_dim * 7 + n_units)
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim)
    scale = rng.uniform(0.05, 1.0, obs_dim).astype(np.float32)
    obs = (rng.standard_normal((256, obs_dim)) * 3).astype(np.float32)
    ok = np.ones(len(obs), bool)
    for sc in (None, scale):
        ref32 = mlp_f16_reference(layers, obs, hact, oact, sc)
        ref64 = mlp_f16_reference(layers, obs, hact, oact, sc, accumulate=np.float64)
        got = mlp_f16_reference(layers, obs, hact, oact, sc, k_block=16, reverse=True)
        assert ref32.dtype == ref64.dtype == got.dtype == np.float32 and got.shape == (256, out_dim)
        E = np.abs(ref32.astype(np.float64) - ref64).max(0)
        err, tol = np.abs(got.astype(np.float64) - ref64).max(0), column_tolerance(E, ref64, ok)
        print('%s scale %s: worst error / tolerance %.3f' % (cfg, sc is not None, float((err / tol).max())))
        assert np.all(err <= tol), (err / tol).max()


def test_restatement_is_exact_where_every_sum_is_and_rounds_as_binary16():
    """small integers and quarters: every order gives the same bits; and the conversions are numpy's astype(float16)"""
    rng = np.random.default_rng(3)
    layers = [(rng.integers(-1, 2, (9, 5)).astype(np.float32), rng.integers(-4, 5, 5).astype(np.float32) / 4),
              (rng.integers(-1, 2, (5, 3)).astype(np.float32), rng.integers(-4, 5, 3).astype(np.float32) / 4)]
    obs = rng.integers(-8, 9, (7, 9)).astype(np.float32) / 4
    want = np.maximum(obs.astype(np.float64) @ layers[0][0] + layers[0][1], 0) @ layers[1][0] + layers[1][1]
    for kw in ({}, {'accumulate': np.float64}, {'k_block': 16, 'reverse': True}, {'k_block': 2}):
        assert np.array_equal(mlp_f16_reference(layers, obs, 'relu', 'linear', **kw), want.astype(np.float32))
    # an input that binary16 cannot hold rounds to nearest even, overflows to inf; a subnormal keeps its value
    one = [(np.ones((1, 1), np.float32), np.zeros(1, np.float32))] * 2
    x = np.array([[2049.0], [2051.0], [65519.0], [65520.0], [2.0 ** -24], [2.0 ** -26]], np.float32)
    assert mlp_f16_reference(one, x, 'linear', 'linear')[:, 0].tolist() == [2048.0, 2052.0, 65504.0, np.inf, 2.0 ** -24, 0.0]


@pytest.mark.parametrize('name', G14)
def test_g14_safe_flags_survive_the_fp16_policy(name):
    """the restatement's actions followed by the oracle's rollout step, five times (hier_decision.py:89-98): punish > 0 equals the
    reference's flags on every start state, for both accumulation orders"""
    g = golden(name)
    task = name.split('_')[-1]
    n = len([k for k in g.files if k.startswith('policy_w')])
    layers = [(g['policy_w%d' % (2 * i)], g['policy_w%d' % (2 * i + 1)]) for i in range(n // 2)]
    host = HostModel(oracle_lib(), task, mode='selecting')
    for kw in ({}, {'k_block': 16, 'reverse': True}):
        obs, punish = g['obs'], np.zeros(len(g['obs']), np.float32)
        for _ in range(5):
            logits = mlp_f16_reference(layers, obs, 'elu', 'linear', g['obs_scale'], **kw)
            obs, out5, _ = host.rollout_step(obs, _tanh_det(logits[:, :2]), path_id=int(g['path_index']))
            punish = punish + out5[3]
        assert np.array_equal(punish > 0, g['safe'] == 0), np.flatnonzero((punish > 0) != (g['safe'] == 0))
