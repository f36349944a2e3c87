"""CPU (-m "not gpu"): the policy-backward family (include/envbuild_mlp_grad.h) is declared as ctypes binds it, lives in a fourth family
table, is exported by the built library next to gfx950 mlp_bwd_data_kernel / mlp_wgrad_kernel, stays out of the hashed forward sources
and is refused by name by the oracle library; and the NumPy restatement of its contract
(env_build_amd.policy_grad.mlp_backward_reference) run in float64 is torch's float64 autograd of a twin built from the same layers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd.policy_grad import mlp_backward_reference
from tests._helpers import ROOT, oracle_lib
from tests._policy_cases import make_layers
from tests.test_policy_f16_host import CONFIGS

HEADER = 'envbuild_mlp_grad.h'
ALL_FAMILIES = ['grad', 'cand', 'cand_grad', 'sample', 'ilqr', 'mlp_f16', 'policy_rollout', 'mlp_grad']


def header_src():
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_declares_what_ctypes_binds():
    text, src = header_src()
    protos = _capi.MLP_GRAD_PROTOTYPES
    assert sorted(protos) == sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert sorted(protos) == ['eb_mlp_backward', 'eb_mlp_backward_workspace_bytes', 'eb_mlp_grad_abi_version', 'eb_mlp_grad_supported',
                              'eb_mlp_param_count', 'eb_mlp_set_params_device']
    for name, (_res, args) in protos.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/%s' % (name, HEADER)
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert len(protos['eb_mlp_backward'][1]) == 12
    assert not set(protos) & set(_capi.PROTOTYPES)
    for table in (_capi.FAMILIES, _capi.MORE_FAMILIES, _capi.POLICY_FAMILIES):
        for row in table.values():
            assert not set(protos) & set(row[5])
    for words in ('NOT part of the contract', 'mlp_backward_reference', 'non-finite', 'bit for bit', 'y > 0 ? 1 : y + 1', 'EB_ESTATE',
                  'Model.get_weights()'):
        assert words in text, words


def test_abi_number_and_the_fourth_family_table():
    _text, src = header_src()
    assert int(re.search(r'#define EB_MLP_GRAD_ABI_VERSION (\d+)', src).group(1)) == _capi.EB_MLP_GRAD_ABI_VERSION == 1
    assert list(_capi.TRAIN_FAMILIES) == ['mlp_grad']
    assert _capi._FAMILY_TABLES == (_capi.FAMILIES, _capi.MORE_FAMILIES, _capi.POLICY_FAMILIES, _capi.TRAIN_FAMILIES)
    row = _capi.TRAIN_FAMILIES['mlp_grad']
    assert len(row) == 6 == len(_capi.FAMILIES['grad'])
    assert row[0] == HEADER and row[3] == 'eb_mlp_grad_abi_version' and row[4] == 1 and row[5] is _capi.MLP_GRAD_PROTOTYPES
    assert [f for table in _capi._FAMILY_TABLES for f in table] == ALL_FAMILIES
    for family in ALL_FAMILIES:
        assert len(_capi.family_row(family)) == 6 and _capi.family_row(family)[3] in _capi.family_row(family)[5]
    assert _capi.family_row('mlp_grad') is row
    with pytest.raises(KeyError):
        _capi.family_row('mlp_grad_f16')


def test_hip_library_exports_the_entries_and_gfx950_kernels():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib, blob = C.CDLL(lib_path), open(lib_path, 'rb').read()
    for name in _capi.MLP_GRAD_PROTOTYPES:
        assert hasattr(lib, name), name
    assert lib.eb_mlp_grad_abi_version() == 1
    assert b'gfx950' in blob
    for kernel in (b'mlp_bwd_data_kernel', b'mlp_wgrad_kernel', b'mlp_wgrad_reduce_kernel', b'mlp_pack_kernel'):
        assert kernel in blob, kernel
    public = os.path.join('..', '..', 'include', HEADER)
    assert 'eb_policy_grad.hip' in eb_build.SOURCES and {'eb_policy_grad.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not set(files) & {'eb_policy_grad.hip', 'eb_policy_grad.h', public}
    # the refusals of a NULL handle need no device: the handle is checked first, and each entry names itself
    lib.eb_last_error.restype = C.c_char_p
    ok, count, size = C.c_int32(7), C.c_int64(7), C.c_size_t(7)
    for name, args in (('eb_mlp_grad_supported', (None, C.byref(ok))), ('eb_mlp_param_count', (None, C.byref(count))),
                       ('eb_mlp_set_params_device', (None, None, None)), ('eb_mlp_backward_workspace_bytes', (None, C.c_int32(4), C.byref(size))),
                       ('eb_mlp_backward', (None, C.c_int32(4), None, None, C.c_int32(0), C.c_float(1.0), None, C.c_size_t(0), None, None, None, None))):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _capi.MLP_GRAD_PROTOTYPES[name]
        assert fn(*args) == -1, name
        assert name.encode() in lib.eb_last_error() and b'null handle' in lib.eb_last_error(), name
    assert ok.value == 7 and count.value == 7 and size.value == 7


def test_the_shared_mlp_device_code_is_written_once():
    """exp_det, tanh_det, elu_det, activate_rt, derivative_rt, the fp32 layer_chain and store_delta are each defined in one file of
    the library, csrc/eb_mlp_device.h, and every policy translation unit includes it, directly or through eb_policy_f16_device.h"""
    text = {f: open(os.path.join(eb_build.CSRC, f)).read() for f in eb_build.SOURCES + eb_build.HEADERS if os.sep not in f}
    for name in ('exp_det', 'tanh_det', 'elu_det', 'activate_rt', 'derivative_rt', 'layer_chain', 'store_delta'):
        # a function definition, under any prefix of the name (ts_exp_det, grad_layer_chain) and after any specifiers or return type
        definition = re.compile(r'^[ \t]*(?:[\w:<>&*]+[ \t]+)+\w*%s[ \t]*\([^;{]*\)\s*\{' % name, re.M)
        assert {f: len(definition.findall(src)) for f, src in text.items() if definition.search(src)} == {'eb_mlp_device.h': 1}, name
    assert 'eb_mlp_device.h' in eb_build.HEADERS and '#include "eb_mlp_device.h"' in text['eb_policy_f16_device.h']
    for unit in ('eb_policy.hip', 'eb_policy_grad.hip', 'eb_policy_rollout_grad.hip', 'eb_policy_f16.hip', 'eb_policy_rollout.hip'):
        assert unit in eb_build.SOURCES
        assert re.search(r'^#include "eb_(mlp|policy_f16)_device\.h"$', text[unit], re.M), unit


def test_the_oracle_library_is_refused_with_the_family_label_and_header():
    api = oracle_lib()
    assert api.backend == 'oracle'
    header, label = _capi.TRAIN_FAMILIES['mlp_grad'][:2]
    assert header == HEADER
    for name in ('mlp_backward', 'mlp_set_params_device', 'mlp_grad_supported', 'mlp_param_count', 'mlp_backward_workspace_bytes',
                 'mlp_grad_abi_version'):
        assert 'eb_' + name in _capi.MLP_GRAD_PROTOTYPES
        with pytest.raises(_capi.EbError) as e:
            getattr(api, name)
        assert label in str(e.value) and header in str(e.value), name
        for fn in (api.mlp_grad_fn, lambda s: api.family_fn('mlp_grad', s)):
            with pytest.raises(_capi.EbError) as e:
                fn('eb_' + name)
            assert label in str(e.value) and header in str(e.value), name
    assert not hasattr(api.lib, 'eb_mlp_backward')


def torch_twin(layers, obs, g, hidden_act, out_act, scale, head, action_range):
    """float64 autograd of a torch network built from the same layers -> (out, g_obs, g_params)"""
    import torch
    acts = {'linear': lambda x: x, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh}
    params = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for pair in layers for a in pair]
    x0 = torch.tensor(np.asarray(obs, np.float64), requires_grad=True)
    x = x0 if scale is None else x0 * torch.tensor(np.asarray(scale, np.float64))
    for L in range(len(layers)):
        x = acts[out_act if L == len(layers) - 1 else hidden_act](x @ params[2 * L] + params[2 * L + 1])
    if head == 1:
        mean = x[:, :x.shape[1] // 2]
        x = action_range * torch.tanh(mean) if action_range > 0 else mean
    (x * torch.tensor(np.asarray(g, np.float64))).sum().backward()
    return x.detach().numpy(), x0.grad.numpy(), [p.grad.numpy() for p in params]


# what tests/test_gpu_policy_grad.py rests on the restatement for, beyond CONFIGS (that module is GPU-marked as a whole; restated here):
# its exact shapes with out_dim 8 .. 32 and obs_dim 192 / 193 / 300 (relu / linear alternating), its wide random configs, and the
# one-term shapes with every hidden activation times every output activation — relu and elu outputs, out_dim 17 / 18 / 32, obs_dim 300
GRAD_CONFIGS = [(16, 2, 64, 8, 'linear', 'linear'), (193, 2, 64, 9, 'relu', 'linear'), (192, 1, 256, 16, 'linear', 'linear'),
                (137, 1, 64, 17, 'relu', 'linear'), (41, 2, 256, 18, 'linear', 'linear'), (45, 3, 128, 24, 'relu', 'linear'),
                (29, 1, 64, 32, 'linear', 'linear'), (300, 1, 128, 4, 'relu', 'linear'),
                (45, 3, 100, 1, 'tanh', 'relu'), (29, 1, 64, 32, 'elu', 'linear'), (137, 2, 128, 17, 'relu', 'tanh'),
                (300, 1, 256, 18, 'elu', 'elu'), (41, 2, 128, 8, 'elu', 'linear'), (41, 3, 100, 1, 'tanh', 'relu')]
GRAD_CONFIGS += [shape + (hact, oact) for shape in ((41, 2, 64, 32), (137, 2, 256, 4), (45, 3, 100, 6))
                 for hact in ('elu', 'tanh', 'relu') for oact in ('linear', 'tanh', 'relu', 'elu')]
ALL_CONFIGS = CONFIGS + GRAD_CONFIGS
ALL_IDS = ['%dx%dx%d_%s' % (c[0], c[1], c[2], c[4]) for c in CONFIGS] + ['%dx%dx%dx%d_%s_%s' % c for c in GRAD_CONFIGS]


@pytest.mark.parametrize('cfg', ALL_CONFIGS, ids=ALL_IDS)
def test_float64_restatement_is_torch_autograd(cfg):
    """both heads, action_range 1.0 / 0.5 / -1.0, scale on and off: every tensor within 1e-12 of its own maximum.  The derivative taken
    from the activation's output is what torch computes for all four activations away from the relu kink."""
    obs_dim, n_hidden, n_units, out_dim, hact, oact = cfg
    assert len(CONFIGS) == 10 and CONFIGS[-1][:4] == (17, 1, 1, 1) and len(set(ALL_IDS)) == len(ALL_IDS) == 60
    rng = np.random.default_rng(obs_dim * 11 + n_units)
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim)
    scale = rng.uniform(0.05, 1.0, obs_dim).astype(np.float32)
    obs = rng.standard_normal((24, obs_dim)).astype(np.float32)
    cases = [(0, 1.0)] + ([(1, 1.0), (1, 0.5), (1, -1.0)] if out_dim % 2 == 0 else [])
    for head, ar in cases:
        g = rng.standard_normal((24, out_dim if head == 0 else out_dim // 2)).astype(np.float32)
        for sc in (None, scale):
            got = mlp_backward_reference(layers, obs, g, hact, oact, sc, head, ar, dtype=np.float64)
            want = torch_twin(layers, obs, g, hact, oact, sc, head, ar)
            pairs = [('out', got[0], want[0]), ('g_obs', got[1], want[1])] + [('g_params[%d]' % k, a, b) for k, (a, b) in enumerate(zip(got[2], want[2]))]
            for what, a, b in pairs:
                assert a.dtype == np.float64 and a.shape == b.shape, what
                assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (what, head, ar, sc is not None)


def test_float32_restatement_is_the_forward_chain_and_close_to_float64():
    """float32: `out` is the deterministic forward (policy.mlp restated with fused multiply-adds), the gradients round as float32 sums"""
    rng = np.random.default_rng(5)
    layers = make_layers(rng, 9, 2, 20, 4)
    obs = rng.standard_normal((16, 9)).astype(np.float32)
    g = rng.standard_normal((16, 4)).astype(np.float32)
    r32 = mlp_backward_reference(layers, obs, g, 'elu', 'linear', dtype=np.float32)
    r64 = mlp_backward_reference(layers, obs, g, 'elu', 'linear', dtype=np.float64)
    assert r32[0].dtype == r32[1].dtype == np.float32 and all(a.dtype == np.float32 for a in r32[2])
    for a, b in zip([r32[0], r32[1]] + r32[2], [r64[0], r64[1]] + r64[2]):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-5 * np.abs(b).max()
    # exact inputs: both dtypes give the same bits
    w = [(rng.integers(-1, 2, (9, 5)).astype(np.float32), rng.integers(-4, 5, 5).astype(np.float32) / 4),
         (rng.integers(-1, 2, (5, 4)).astype(np.float32), rng.integers(-4, 5, 4).astype(np.float32) / 4)]
    o = rng.integers(-8, 9, (7, 9)).astype(np.float32) / 4
    gg = rng.integers(-4, 5, (7, 2)).astype(np.float32) / 4
    for head, gx in ((0, np.concatenate([gg, gg], 1)), (1, gg)):
        e32 = mlp_backward_reference(w, o, gx, 'relu', 'linear', None, head, -1.0, dtype=np.float32)
        e64 = mlp_backward_reference(w, o, gx, 'relu', 'linear', None, head, -1.0, dtype=np.float64)
        for a, b in zip([e32[0], e32[1]] + e32[2], [e64[0], e64[1]] + e64[2]):
            assert np.array_equal(a.astype(np.float64), b)
