"""Shared by tests/test_epoch_host.py and tests/test_gpu_epoch.py (a helper module like _ppo.py and _capture.py: pytest does not collect
it, and importing it touches no device): the header's structs as ctypes field lists, the epoch library built and bound, the two small
networks and the iteration data of the PPOEpochs tests."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import epoch
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_epoch.h')
KERNELS = ('adv_stats_fold_kernel', 'adv_stats_partial_kernel', 'epoch_advance_kernel', 'minibatch_gather_kernel', 'ppo_log_kernel')
ENTRIES = ('eb_minibatch_gather', 'eb_adv_stats', 'eb_ppo_log', 'eb_epoch_advance')
UNIT = ('eb_epoch.hip', 'eb_epoch.h', 'eb_epoch_device.h')
SCALARS = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'float': C.c_float, 'double': C.c_double}


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def struct_fields(src, name, nested=(), macros=()):
    """`typedef struct name { ... } name;` -> [(field, ctype)] in order; a pointer is c_void_p, `a, b` declares two fields of one type"""
    nested, macros = dict(nested), dict(macros)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        if not decl.strip():
            continue
        first, *more = [p.strip() for p in decl.split(',')]
        m = re.match(r'(.*?)(\w+)(\[(\w+)\])?$', first)
        kind = m.group(1).replace('const ', '').strip()
        kind = C.c_void_p if kind.endswith('*') else nested[kind] if kind in nested else SCALARS[kind]
        if m.group(4):
            kind = kind * macros[m.group(4)]
        fields.append((m.group(2), kind))
        fields += [(p, kind) for p in more]
    return fields


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_epoch.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, its bytes)"""
    path = eb_build.build_epoch()
    assert not eb_build.epoch_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.epoch_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in epoch.EPOCH_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


# ---- the PPOEpochs case: 41 -> 64 -> 64 -> 4 and 41 -> 64 -> 64 -> 1, 65 rows, N = 4 * 65 + 3, 2 epochs of 4 minibatches ----
POLICY_CFG, VALUE_CFG = (41, 2, 64, 4, 'elu', 'linear'), (41, 2, 64, 1, 'elu', 'relu')
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8
PPO_KW = dict(action_range=1.0, clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)
ROWS, EPOCHS, MINIBATCHES = 65, 2, 4
N = MINIBATCHES * ROWS + 3
SEED = 11
FIELDS = ('obs', 'actions', 'logp_old', 'adv', 'ret', 'v_old')


def make_nets():
    """the two networks, the same weights at every call (make_net's generator is seeded by the configuration); the policy's output layer
    times 0.4 (means of a few tenths), the value head's bias positive (the relu is alive on most rows)"""
    from env_build_amd.policy_grad import TrainableMLPNet
    from tests._ppo import make_net
    policy, p_layers, scale = make_net(POLICY_CFG, True, TrainableMLPNet)
    p_layers = list(p_layers)
    p_layers[-1] = ((p_layers[-1][0] * np.float32(0.4)).astype(np.float32), p_layers[-1][1])
    policy.set_weights([a for pair in p_layers for a in pair])
    value, v_layers, _ = make_net(VALUE_CFG, False, TrainableMLPNet)
    v_layers = list(v_layers)
    v_layers[-1] = (v_layers[-1][0], (np.abs(v_layers[-1][1]) + np.float32(1.0)).astype(np.float32))
    value.set_weights([a for pair in v_layers for a in pair])
    value.set_obs_scale(scale)
    return policy, value


def make_data(policy, n=N, seed=5):
    """one iteration's tensors on the device: observations N(0, 1), the actions the sampler draws under the policy, logp_old from
    eb_policy_logp on the same weights (so the first minibatch's ratio is exactly 1), advantages off centre, returns around v_old"""
    import torch
    from env_build_amd.policy_logp import log_prob_actions
    from env_build_amd.policy_sample import sample_actions
    from tests._ppo import gpu
    rng = np.random.default_rng(seed)
    obs = gpu(rng.standard_normal((n, 41)))
    actions = sample_actions(policy, obs, 1.0, seed=seed, counter=0, want=())['actions'].t.clone()
    logp_old = log_prob_actions(policy, obs, actions, 1.0)['logp'].t.clone()
    v_old = (1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    ret = (v_old + rng.uniform(-0.6, 0.6, n)).astype(np.float32)
    adv = (0.3 + 1.7 * rng.standard_normal(n)).astype(np.float32)
    torch.cuda.synchronize()
    return dict(obs=obs, actions=actions.contiguous(), logp_old=logp_old.contiguous(), adv=gpu(adv), ret=gpu(ret), v_old=gpu(v_old))


def snapshot(upd):
    """every parameter, m, v, the Adam state and rows.* of a PPOUpdate, on the host"""
    import torch
    torch.cuda.synchronize()
    out = {'policy': upd.policy._flat.detach().cpu().numpy().copy(), 'value': upd.value._flat.detach().cpu().numpy().copy()}
    for k in range(2):
        out['m%d' % k], out['v%d' % k] = upd.adam.m[k].cpu().numpy().copy(), upd.adam.v[k].cpu().numpy().copy()
    for name in ('logp', 'ratio', 'surr', 'ent', 'vloss'):
        out[name] = getattr(upd.rows, name).cpu().numpy().copy()
    out['state'] = upd.adam.state.buffer.cpu().numpy().copy()
    return out
