"""Shared by tests/test_ac_host.py and tests/test_gpu_ac.py (a helper module like _ctl.py and _collect.py: pytest does not collect it, and
importing it touches no device): the actor-critic library built and bound, the rows of the loss and sampling cases with the branch each
row takes, device outputs cut from the middle of sentinel allocations, the shared network of the update tests and its data."""
import ctypes as C
import functools
import os

import numpy as np

from env_build_amd import ac
from env_build_amd import build as eb_build
from tests import _ctl
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_ac.h')
KERNELS = ('ac_loss_kernel', 'ac_sample_kernel')
ENTRIES = ('eb_ac_loss', 'eb_ac_sample')
UNIT = ('eb_ac.hip', 'eb_ac.h')
SIZES = (1, 63, 64, 65, 257)
ACT_DIMS = (1, 2, 15)
RANGES = (1.0, 0.3, -1.0)
SENTINEL = -77.25
SLACK = 5                                                          # an odd number of floats on both sides: 4-byte alignment only
ADV_NORM = (0.05, 1.3)
CLIP, CLIP_V, ENT_COEF, VF_COEF = 0.2, 0.2, 1e-3, 0.5
NAN_LOGIT_ROW, NAN_VALUE_ROW, NAN_OLD_ROW = 5, 7, 9                # planted with n >= 63
BRANCHES = ('inside', 'above_blocked', 'above_open', 'below_blocked', 'below_open', 'v_inside', 'v_outside', 'v_first', 'v_second_outside')


def header():
    """(the header's text, the same without comments)"""
    import re
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


struct_fields = _ctl.struct_fields


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_ac.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, its bytes)"""
    path = eb_build.build_ac()
    assert not eb_build.ac_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.ac_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in ac.AC_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


def same(a, b):
    """bit for bit; a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the rows ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_case(n, act_dim, action_range):
    """n rows of y [n, 2A + 1], actions, logp_old, adv, ret, v_old.  Means of a few tenths, log-std in [-1.5, 0.5], the action the
    sampler's restatement draws, values around 1.  Row i's logp_old is the restatement's logp shifted by the i % 5-th of (0, -0.5, -0.5,
    +0.5, +0.5) — inside the clip interval, above it and below it — and its advantage has the sign that blocks or opens the clamp under
    both adv_norm (0.05, 1.3) and none; its v_old is the value shifted by the (i // 5) % 4-th of (+0.05, -0.05, +0.5, -0.5) — inside and
    outside clip_v — and its return makes the clipped square the larger one (l2 > l1: outside, the gradient is 0) or not (l2 <= l1: the
    unclipped error's).  Inside the interval the clipped value is the value up to a rounding, so which square is larger there is not
    planned.  With n >= 63, three rows carry a NaN: in a logit, in
    the value column, in logp_old."""
    from env_build_amd import policy_sample as ps
    from env_build_amd import ppo
    rng = np.random.default_rng(1000 * n + 10 * act_dim + int(10 * abs(action_range)))
    W = 2 * act_dim + 1
    y = np.empty((n, W), np.float32)
    y[:, :act_dim] = 0.3 * rng.standard_normal((n, act_dim))
    y[:, act_dim:2 * act_dim] = rng.uniform(-1.5, 0.5, (n, act_dim))
    y[:, 2 * act_dim] = 1.0 + 0.5 * rng.standard_normal(n)
    eps = rng.standard_normal((n, act_dim)).astype(np.float32)
    actions = ps.policy_sample_reference(y[:, :2 * act_dim], eps, action_range)[0]
    i = np.arange(n)
    logp = ppo.ppo_reference(y[:, :2 * act_dim], actions, np.zeros(n, np.float32), np.zeros(n, np.float32), action_range, CLIP)['logp']
    shift = np.array([0.0, -0.5, -0.5, 0.5, 0.5], np.float32)[i % 5]        # logp - logp_old = -shift: ratio 1, e^0.5, e^0.5, e^-0.5, e^-0.5
    logp_old = (logp + shift).astype(np.float32)
    sign = np.array([1.0, 1.0, -1.0, -1.0, 1.0], np.float32)[i % 5]         # above & A > 0: blocked; above & A < 0: open; below & A < 0: blocked
    adv = (sign * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    v = y[:, 2 * act_dim]
    dv = np.array([0.05, -0.05, 0.5, -0.5], np.float32)[(i // 5) % 4]       # v - v_old
    v_old = (v - dv).astype(np.float32)
    # ret on the far side of v_old from v: the clipped value is nearer to it than v, l2 < l1 (first); on the near side: l2 > l1 (second)
    far = ((i // 20) % 2).astype(bool)
    ret = np.where(far, v_old - np.sign(dv) * np.float32(1.0), v + np.sign(dv) * np.float32(1.0)).astype(np.float32)
    if n >= 63:
        y[NAN_LOGIT_ROW, 0] = np.nan
        y[NAN_VALUE_ROW, 2 * act_dim] = np.nan
        logp_old[NAN_OLD_ROW] = np.nan
    return dict(y=y, actions=actions, logp_old=logp_old, adv=adv, ret=ret, v_old=v_old, eps=eps)


def loss_reference(case, action_range, clip, with_norm, with_v_old):
    n = case['y'].shape[0]
    return ac.ac_loss_reference(case['y'], case['actions'], case['logp_old'], case['adv'], case['ret'], action_range, clip, ent_coef=ENT_COEF,
                                scale=1.0 / n, adv_norm=ADV_NORM if with_norm else None, v_old=case['v_old'] if with_v_old else None,
                                clip_v=CLIP_V, v_scale=VF_COEF / n)


def branches(case, ref, clip):
    """the rows of each branch, from the restatement's ratio and normalised advantage and the case's values (selects on fp32 numbers; the
    classification of the rows, not a second statement of the loss)"""
    f = np.float32
    r, A = ref['ratio'], ref['A']
    lo, hi = f(1) - f(clip), f(1) + f(clip)
    with np.errstate(all='ignore'):
        s1, s2 = r * A, np.where(r < lo, lo, np.where(r > hi, hi, r)) * A
        blocked = ((r < lo) | (r > hi)) & (s2 <= s1)
        A2 = case['y'].shape[1] - 1
        v = case['y'][:, A2]
        dv = v - case['v_old']
        inside = (dv >= -f(CLIP_V)) & (dv <= f(CLIP_V))
        outside = (dv < -f(CLIP_V)) | (dv > f(CLIP_V))
        e = v - case['ret']
        e2 = (case['v_old'] + np.clip(dv, -f(CLIP_V), f(CLIP_V))) - case['ret']
        second = e2 * e2 > e * e
        first = e2 * e2 <= e * e
    return dict(inside=(r >= lo) & (r <= hi), above_blocked=(r > hi) & blocked, above_open=(r > hi) & ~blocked, below_blocked=(r < lo) & blocked,
                below_open=(r < lo) & ~blocked, v_inside=inside, v_outside=outside, v_first=first, v_second_outside=outside & second)


def every_branch_is_taken(case, ref, clip, with_v_old):
    """with n >= 63 every branch has a row (with clip = 0 only ratio exactly 1 is inside; a single row is one branch)"""
    taken = {k: int(m.sum()) for k, m in branches(case, ref, clip).items()}
    wanted = [k for k in BRANCHES if with_v_old or not k.startswith('v_')]
    return [k for k in wanted if not taken[k]]


# ---- device buffers ------------------------------------------------------------------------------------------------------------------------
class Out(object):
    """a float32 device array of `shape` in the MIDDLE of a larger allocation, SLACK sentinel floats on both sides, itself filled with the
    sentinel; host() -> (the array, whether the slack is as made)"""

    def __init__(self, *shape):
        import torch
        self.shape, self.size = shape, int(np.prod(shape))
        self.big = torch.full((self.size + 2 * SLACK,), SENTINEL, dtype=torch.float32, device='cuda')
        self.t = self.big[SLACK:SLACK + self.size].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        raw = self.big.cpu().numpy()
        ok = bool((raw[:SLACK] == SENTINEL).all() and (raw[SLACK + self.size:] == SENTINEL).all())
        return raw[SLACK:SLACK + self.size].reshape(self.shape).copy(), ok


def gpu(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- the shared network of the update tests: 41 -> 64 -> 64 -> 5 ----------------------------------------------------------------------------
NET_CFG = (41, 2, 64, 5, 'elu', 'linear')
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8
PPO_KW = dict(action_range=1.0, clip=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF, clip_v=CLIP_V, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.5)


@functools.lru_cache(maxsize=None)
def net_layers(cfg=NET_CFG):
    """the layers and the observation scale of the shared network without a device: tests/_ppo.make_net's recipe (its generator, seeded by
    the configuration), the logit columns of the output layer times 0.4 (means of a few tenths) and the value column's bias 1"""
    from tests._policy_cases import make_layers
    obs_dim, n_hidden, units, out_dim = cfg[:4]
    rng = np.random.default_rng(sum(cfg[:4]))
    layers = list(make_layers(rng, obs_dim, n_hidden, units, out_dim, bias_scale=0.3))
    scale = rng.uniform(0.25, 1.0, obs_dim).astype(np.float32)
    kernel, bias = layers[-1][0].copy(), layers[-1][1].copy()
    kernel[:, :out_dim - 1] *= np.float32(0.4)
    kernel[:, out_dim - 1] *= np.float32(0.1)
    bias[out_dim - 1] = np.float32(1.0)
    layers[-1] = (kernel.astype(np.float32), bias.astype(np.float32))
    return layers, scale


def make_net(cfg=NET_CFG, scale=None):
    """the shared TrainableMLPNet of `cfg`, the same weights at every call"""
    layers, sc = net_layers(cfg)
    net = ac.make_net(cfg[0], cfg[1], cfg[2], cfg[4], (cfg[3] - 1) // 2)
    net.set_weights([a for pair in layers for a in pair])
    net.set_obs_scale(sc if scale is None else scale)
    return net


def make_data(net, n, seed=5, shift=0.0):
    """n rows on the device: observations N(0, 1), the actions the sampler draws under the split policy, logp_old from eb_policy_logp on
    the same weights (+ up to +-shift), advantages off centre, v_old around the net's value, returns around v_old"""
    import torch
    from env_build_amd.policy_logp import log_prob_actions
    from env_build_amd.policy_sample import sample_actions
    policy, value = ac.split(net)
    rng = np.random.default_rng(seed)
    obs = gpu(rng.standard_normal((n, net.input_dim)))
    actions = sample_actions(policy, obs, 1.0, seed=seed, counter=0, want=())['actions'].t.clone()
    logp_old = log_prob_actions(policy, obs, actions, 1.0)['logp'].t.clone()
    if shift:
        logp_old += gpu(rng.uniform(-shift, shift, n))
    v = value.call(obs).t[:, 0].clone()
    v_old = v + gpu(0.3 * rng.standard_normal(n))
    ret = v_old + gpu(rng.uniform(-0.6, 0.6, n))
    adv = gpu(0.3 + 1.7 * rng.standard_normal(n))
    torch.cuda.synchronize()
    return dict(obs=obs, actions=actions.contiguous(), logp_old=logp_old.contiguous(), adv=adv, ret=ret.contiguous(), v_old=v_old.contiguous())


def fill(upd, data, rows=None):
    rows = slice(0, upd.n) if rows is None else rows
    for k in ('obs', 'actions', 'logp_old', 'adv', 'ret', 'v_old'):
        getattr(upd.mb, k).copy_(data[k][rows])
    upd.mb.adv_norm.copy_(gpu(np.array(ADV_NORM, np.float32)))


def snapshot(upd):
    """the parameters, m, v, the Adam state and rows.* of an update over ONE net, on the host"""
    import torch
    torch.cuda.synchronize()
    out = {'net': upd.policy._flat.detach().cpu().numpy().copy(), 'm': upd.adam.m[0].cpu().numpy().copy(), 'v': upd.adam.v[0].cpu().numpy().copy(),
           'state': upd.adam.state.buffer.cpu().numpy().copy()}
    for name in ('logp', 'ratio', 'surr', 'ent', 'vloss'):
        out[name] = getattr(upd.rows, name).cpu().numpy().copy()
    return out


def differing(a, b):
    return [k for k in a if not (same(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k]))]
