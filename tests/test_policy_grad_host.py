"""CPU (-m "not gpu"): the shared MLP device code is defined once, and the NumPy restatement of the policy backward's contract
(env_build_amd.policy_grad.mlp_backward_reference, include/envbuild_mlp_grad.h) run in float64 is torch's float64 autograd of a twin
built from the same layers.  (The family's ABI: tests/test_family_abi.py.)"""
import os
import re

import numpy as np
import pytest

from env_build_amd import build as eb_build
from env_build_amd.policy_grad import mlp_backward_reference
from tests._policy_cases import HOST_CONFIGS as CONFIGS, make_layers, torch_twin


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


# what tests/test_gpu_policy_grad.py rests on the restatement for, beyond CONFIGS:
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
