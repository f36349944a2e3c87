"""GPU (-m gpu): the PPO family (include/envbuild_ppo.h) — the surrogate row alone against the float32 restatement bit for bit, the fused
launch against eb_mlp_forward followed by the row and against eb_policy_logp, the first pass (ratio exactly 1, g_logits from
eb_policy_logp_vjp), optional outputs and refusals, row independence, eb_gae against its restatement and against the torch loop of
examples/ppo_env_loop.py, `policy_loss` on a TrainableMLPNet against the float64 torch twin, the three entries on a side stream and
under capture, and the example."""
import ctypes as C
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd import ppo
from env_build_amd.policy_grad import mlp_backward_reference
from tests._capture import capture, side_stream
from tests._helpers import ROOT
from tests._policy import SENTINEL, same
from tests._ppo import FUSED_CONFIGS, N_MAX, example_loop, gpu, host, logits_case, make_net

pytestmark = pytest.mark.gpu

RANGES = (1.0, 0.5, None)
SIZES = (1, 63, 64, 65, N_MAX)
SCALE = 1.0 / 64.0
ENT_COEF = 1e-3
OPTIONAL = ('ratio', 'surr', 'ent', 'g_logits', 'z_out')
KEYS = ('logp', 'ratio', 'surr', 'ent', 'g_logits', 'z')


def ar_of(action_range):
    return -1.0 if action_range is None else action_range


def raw_args(stream, n, out_dim=0, action_range=1.0, clip=0.2, ent_coef=ENT_COEF, scale=SCALE, **tensors):
    return ppo._args(stream, n, out_dim, ar_of(action_range), clip, ent_coef, scale, **tensors)


# ---- 1: the row alone against the restatement ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_case(out_dim, action_range):
    """tests/_ppo.logits_case, which is tests/test_gpu_policy_logp.py's (the action set at, beyond and inside +-action_range, +-0, 1e-30; log-std from -20 to 5 and
    beyond the exponential's clamps; a NaN row, an inf row, a NaN action) with logp_old = logp - d: d cycles through 0 (r == 1),
    log 0.6, log 0.95, log 1.5 and, on rows 101, 102, 103 and 106, +-100 and +-88.5 (beyond both clamps of exp_det); advantages of both signs, zeros of both
    signs outside the interval (rows 105, 107), a NaN (row 110), a NaN logp_old (row 113)"""
    logits, actions, _, want = logits_case(out_dim, action_range)
    rng = np.random.default_rng(1000 + out_dim)
    d = np.log(np.array([1.0, 0.6, 0.95, 1.5]))[np.arange(N_MAX) % 4]
    d[[101, 102, 103, 106]] = [100.0, -100.0, 88.5, -88.5]
    with np.errstate(all='ignore'):
        logp_old = (want['logp'].astype(np.float64) - d).astype(np.float32)
    logp_old[np.arange(N_MAX) % 4 == 0] = want['logp'][np.arange(N_MAX) % 4 == 0]
    adv = rng.standard_normal(N_MAX).astype(np.float32)
    adv[105], adv[107], adv[110], logp_old[113] = 0.0, -0.0, np.nan, np.nan
    adv_norm = np.array([0.25, 1.5], np.float32)
    return logits, actions, logp_old, adv, adv_norm


@functools.lru_cache(maxsize=None)
def row_want(out_dim, action_range, clip, normed):
    logits, actions, logp_old, adv, adv_norm = row_case(out_dim, action_range)
    return ppo.ppo_reference(logits, actions, logp_old, adv, action_range, clip, ENT_COEF, scale=SCALE, adv_norm=adv_norm if normed else None)


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('out_dim', [2, 4, 6, 32])
def test_from_logits_is_the_restatement_bit_for_bit(out_dim, action_range):
    import torch
    logits, actions, logp_old, adv, adv_norm = row_case(out_dim, action_range)
    for clip in (0.0, 0.2):
        for normed in (True, False):
            want = row_want(out_dim, action_range, clip, normed)
            for n in SIZES:
                got = host(ppo.surrogate_from_logits(gpu(logits[:n]), actions[:n], logp_old[:n], adv[:n], action_range, clip, ENT_COEF,
                                                     adv_norm if normed else None, want=('ratio', 'surr', 'ent', 'g_logits', 'z'), scale=SCALE))
                for k in KEYS:
                    assert same(got[k], want[k][:n]), '%s differs, n %d, clip %g, adv_norm %s' % (k, n, clip, normed)
    want = row_want(out_dim, action_range, 0.2, True)
    # the ratio is what exp_det returns beyond its clamps; the poisoned rows poison themselves only
    r = want['ratio']
    first = (np.arange(N_MAX) % 4 == 0) & np.isfinite(want['logp'])
    assert first.sum() > 60 and (r[first] == 1.0).all()
    assert r[101] == r[103] and r[102] == r[106] and 1e38 < r[101] < np.inf and 0 < r[102] < 1e-37
    for row in (110, 113):
        assert np.isnan(want['surr'][row]) and np.isnan(want['g_logits'][row]).all()
    free = row_want(out_dim, action_range, 0.2, False)                # A == 0 outside the interval, on both sides
    assert free['g_lp'][105] == 0.0 and free['g_lp'][107] == 0.0 and free['ratio'][105] < 0.8 and free['ratio'][107] > 1.2
    assert np.isfinite(want['g_logits'][[105, 107, 109, 111, 112]]).all()
    # each optional output NULL in turn: the others as before, nothing beyond their n rows
    n = 65
    stream = torch.cuda.current_stream().cuda_stream
    y, a, lo, ad, an = gpu(logits[:n]), gpu(actions[:n]), gpu(logp_old[:n]), gpu(adv[:n]), gpu(adv_norm)
    widths = dict(logp=1, ratio=1, surr=1, ent=1, g_logits=out_dim, z_out=out_dim // 2)
    for skip in OPTIONAL + (None,):
        outs = {k: torch.full(((n + 1) * w,), SENTINEL, device='cuda') for k, w in widths.items()}
        given = {k: t for k, t in outs.items() if k != skip}
        ppo._call(pl._capi.hip_api(), 'eb_ppo_surrogate_from_logits',
                  C.byref(raw_args(stream, n, out_dim, action_range, logits=y, actions=a, logp_old=lo, adv=ad, adv_norm=an, **given)))
        torch.cuda.synchronize()
        for k, w in widths.items():
            t = outs[k].cpu().numpy()
            if k == skip:
                assert (t == SENTINEL).all(), k
            else:
                assert same(t[:n * w], want[k.replace('_out', '')][:n].reshape(-1)) and (t[n * w:] == SENTINEL).all(), (k, skip)


# ---- 2, 3: the fused launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', FUSED_CONFIGS, ids=['%dx%dx%dx%d' % c[:4] for c in FUSED_CONFIGS])
def test_fused_equals_forward_then_from_logits_and_the_first_pass_has_ratio_one(cfg):
    obs_dim, out_dim = cfg[0], cfg[3]
    act_dim = out_dim // 2
    rng = np.random.default_rng(1)
    n = 129                                                        # two full blocks and a one-row tail
    obs = rng.standard_normal((n, obs_dim)).astype(np.float32)
    actions = rng.uniform(-1.2, 1.2, (n, act_dim)).astype(np.float32)             # inside and beyond both ranges
    adv = rng.standard_normal(n).astype(np.float32)
    adv_norm = np.array([0.1, 1.25], np.float32)
    d = np.log(np.array([1.0, 0.6, 0.95, 1.5], np.float32))[np.arange(n) % 4]
    every = ('ratio', 'surr', 'ent', 'g_logits', 'logits', 'z')
    for scale in (False, True):
        net, _, _ = make_net(cfg, scale)
        logits = net.call(obs)
        for ar in RANGES:
            lp = host(pl.log_prob_actions(net, obs, actions, ar, want=('logits', 'z')))
            logp_old = (lp['logp'] - d).astype(np.float32)
            want = host(ppo.surrogate_from_logits(logits, actions, logp_old, adv, ar, 0.2, ENT_COEF, adv_norm, want=every[:4] + ('z',)))
            got = host(ppo.surrogate(net, obs, actions, logp_old, adv, ar, 0.2, ENT_COEF, adv_norm, want=every))
            assert same(got['logits'], logits.numpy()) and same(got['logits'], lp['logits']), 'logits_out, range %r' % (ar,)
            assert same(got['logp'], lp['logp']) and same(got['z'], lp['z']), 'logp / z against eb_policy_logp, range %r' % (ar,)
            for k in want:
                assert same(got[k], want[k]), '%s, range %r, scale %s' % (k, ar, scale)
            # the first pass: logp_old from eb_policy_logp on the same handle
            first = host(ppo.surrogate(net, obs, actions, lp['logp'], adv, ar, 0.2, ENT_COEF, adv_norm, want=('ratio', 'surr', 'g_logits')))
            assert (first['ratio'] == 1.0).all(), 'first-pass ratio, range %r' % (ar,)
            sc = np.float32(1.0 / n)
            A = (adv - adv_norm[0]) * adv_norm[1]
            assert same(first['surr'], A)
            g = pl.log_prob_vjp(gpu(lp['logits']), lp['z'], ((-sc) * A) * np.float32(1.0)).numpy()
            g[:, act_dim:] = g[:, act_dim:] + (-(sc * np.float32(ENT_COEF)))
            assert same(first['g_logits'], g), 'first-pass g_logits against eb_policy_logp_vjp, range %r' % (ar,)


# ---- 4: rows are independent, calls repeat, refusals write nothing ------------------------------------------------------------------------
def test_rows_are_independent_and_calls_repeat():
    cfg = (137, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True)
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((N_MAX, 137)).astype(np.float32)
    actions = rng.uniform(-1.0, 1.0, (N_MAX, 2)).astype(np.float32)
    adv = rng.standard_normal(N_MAX).astype(np.float32)
    adv_norm = np.array([0.1, 1.25], np.float32)
    logp_old = host(pl.log_prob_actions(net, obs, actions, 1.0))['logp'] - rng.uniform(-0.5, 0.5, N_MAX).astype(np.float32)
    every = ('ratio', 'surr', 'ent', 'g_logits', 'logits', 'z')
    call = lambda rows: host(ppo.surrogate(net, obs[rows], actions[rows], logp_old[rows], adv[rows], 1.0, 0.2, ENT_COEF, adv_norm,
                                           want=every, scale=SCALE))
    full, again = call(slice(None)), call(slice(None))
    for k in full:
        assert same(full[k], again[k]), k
    assert (full['ratio'] < 0.8).any() and (full['ratio'] > 1.2).any() and ((full['ratio'] > 0.8) & (full['ratio'] < 1.2)).any()
    perm = rng.permutation(N_MAX)
    mixed = call(perm)
    for k in full:
        assert same(mixed[k], full[k][perm]), k
    alone = host(ppo.surrogate_from_logits(gpu(full['logits'])[perm], actions[perm], logp_old[perm], adv[perm], 1.0, 0.2, ENT_COEF, adv_norm,
                                           want=every[:4] + ('z',), scale=SCALE))
    for k in alone:
        assert same(alone[k], full[k][perm]), k
    for row in (0, 63, 64, 200, N_MAX - 1):
        one = call(slice(row, row + 1))
        for k in full:
            assert same(one[k], full[k][row:row + 1]), '%s, row %d' % (k, row)


def test_refusals_and_empty_batches_write_nothing():
    import torch
    cfg = (41, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True)
    rng = np.random.default_rng(4)
    n = 130
    x, a = gpu(rng.standard_normal((n, 41))), gpu(rng.uniform(-1.0, 1.0, (n, 2)))
    lo, ad, an = gpu(rng.standard_normal(n)), gpu(rng.standard_normal(n)), gpu(np.array([0.0, 1.0]))
    y = net.call(x).t
    stream = torch.cuda.current_stream().cuda_stream
    fns = ppo.bind(net.api)
    new = lambda *shape: torch.full(shape, SENTINEL, device='cuda')
    outs = dict(logp=new(n), ratio=new(n), surr=new(n), ent=new(n), g_logits=new(n, 4), logits_out=new(n, 4), z_out=new(n, 2))
    ins = dict(obs=x, actions=a, logp_old=lo, adv=ad, adv_norm=an)
    alone = dict(ins, logits=y)
    nan = float('nan')
    without = lambda d, k: dict(d, **{k: None})
    refusals = [
        ('eb_ppo_surrogate', raw_args(stream, n, 0, nan, **ins, **outs)),
        ('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, clip=nan, **ins, **outs)),
        ('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, clip=-0.5, **ins, **outs)),
        ('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, ent_coef=nan, **ins, **outs)),
        ('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, scale=nan, **ins, **outs)),
        ('eb_ppo_surrogate', raw_args(stream, -1, 0, 1.0, **ins, **outs)),
    ] + [('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, **without(ins, k), **outs)) for k in ('obs', 'actions', 'logp_old', 'adv')] + [
        ('eb_ppo_surrogate', raw_args(stream, n, 0, 1.0, **ins, **without(outs, 'logp'))),
        ('eb_ppo_surrogate_from_logits', raw_args(stream, n, 3, 1.0, **alone, **outs)),
        ('eb_ppo_surrogate_from_logits', raw_args(stream, n, 34, 1.0, **alone, **outs)),
        ('eb_ppo_surrogate_from_logits', raw_args(stream, n, 4, nan, **alone, **outs)),
        ('eb_ppo_surrogate_from_logits', raw_args(stream, n, 4, 1.0, **without(alone, 'logits'), **outs)),
        ('eb_ppo_surrogate_from_logits', raw_args(stream, n, 4, 1.0, **without(alone, 'logp_old'), **outs)),
    ]
    for name, struct in refusals:
        with pytest.raises(ValueError, match=name + ':'):
            if name == 'eb_ppo_surrogate':
                net.api.check(fns[name](net._handle, C.byref(struct)))
            else:
                net.api.check(fns[name](C.byref(struct)))
    ppo._call(net.api, 'eb_ppo_surrogate', net._handle, C.byref(raw_args(stream, 0, 0, 1.0, **outs)))
    ppo._call(net.api, 'eb_ppo_surrogate_from_logits', C.byref(raw_args(stream, 0, 4, 1.0, **outs)))
    # eb_gae: refusals and n = 0
    T = 3
    g_in = dict(rewards=new(T, n), values=new(T, n), v_last=new(n), nonterminal=new(T, n))
    g_out = dict(adv=new(T, n), ret=new(T, n))
    gae_refusals = [ppo._gae_args(stream, 0, n, 0.99, 0.95, **g_in, **g_out), ppo._gae_args(stream, 65536, n, 0.99, 0.95, **g_in, **g_out),
                    ppo._gae_args(stream, T, -1, 0.99, 0.95, **g_in, **g_out), ppo._gae_args(stream, T, n, nan, 0.95, **g_in, **g_out),
                    ppo._gae_args(stream, T, n, 0.99, float('inf'), **g_in, **g_out),
                    ppo._gae_args(stream, T, n, 0.99, 0.95, **without(g_in, 'v_last'), **g_out),
                    ppo._gae_args(stream, T, n, 0.99, 0.95, **without(g_in, 'rewards'), **g_out),
                    ppo._gae_args(stream, T, n, 0.99, 0.95, **g_in, **without(g_out, 'adv'))]
    for struct in gae_refusals:
        with pytest.raises(ValueError, match='eb_gae:'):
            net.api.check(fns['eb_gae'](C.byref(struct)))
    ppo._call(net.api, 'eb_gae', C.byref(ppo._gae_args(stream, T, 0, 0.99, 0.95, **g_out)))
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(g_out.values()):
        assert bool((t == SENTINEL).all())
    empty = ppo.surrogate(net, np.zeros((0, 41), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32),
                          1.0, 0.2, want=('ratio', 'g_logits'))
    assert empty['logp'].numpy().shape == (0,) and empty['g_logits'].numpy().shape == (0, 4)


def test_an_fp16_handle_is_refused_by_the_fused_entry_and_served_by_surrogate():
    import torch
    cfg = (41, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True, precision='fp16')
    rng = np.random.default_rng(4)
    n = 130
    obs, actions = rng.standard_normal((n, 41)).astype(np.float32), rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    logp_old, adv = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ok = C.c_int32(7)
    ppo._call(net.api, 'eb_ppo_surrogate_supported', net._handle, C.byref(ok))
    assert ok.value == 0 and b'eb_ppo_surrogate: ' in net.api.lib.eb_last_error() and b'EB_MLP_PRECISION_F32' in net.api.lib.eb_last_error()
    logp = torch.full((n,), SENTINEL, device='cuda')
    with pytest.raises(ValueError, match='eb_ppo_surrogate: the handle.s precision must be EB_MLP_PRECISION_F32'):
        ppo._call(net.api, 'eb_ppo_surrogate', net._handle,
                  C.byref(raw_args(torch.cuda.current_stream().cuda_stream, n, 0, 1.0, obs=gpu(obs), actions=gpu(actions), logp_old=gpu(logp_old),
                                   adv=gpu(adv), logp=logp)))
    torch.cuda.synchronize()
    assert bool((logp == SENTINEL).all())
    logits = net.call(obs)
    every = ('ratio', 'surr', 'ent', 'g_logits', 'z')
    want = host(ppo.surrogate_from_logits(logits, actions, logp_old, adv, 1.0, 0.2, ENT_COEF, want=every))
    got = host(ppo.surrogate(net, obs, actions, logp_old, adv, 1.0, 0.2, ENT_COEF, want=every + ('logits',)))
    assert same(got['logits'], logits.numpy())
    for k in want:
        assert same(got[k], want[k]), k
    got = host(ppo.surrogate(lambda o: net.call(o), obs, actions, logp_old, adv, 1.0, 0.2, ENT_COEF, want=every))
    for k in want:
        assert same(got[k], want[k]), k


# ---- 5: generalised advantage estimation ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gae_case(T):
    rng = np.random.default_rng(50 + T)
    n = N_MAX
    rewards, values, nv = (rng.standard_normal((T, n)).astype(np.float32) for _ in range(3))
    v_last = rng.standard_normal(n).astype(np.float32)
    live = (rng.uniform(size=(T, n)) > 0.15).astype(np.float32)
    live[0, :8:2] = 0.0
    live[T - 1, 1:9:2] = 0.0
    carry = live.copy()
    flip = rng.uniform(size=(T, n)) < 0.1
    carry[flip] = 1.0 - carry[flip]
    return rewards, values, v_last, live, nv, carry


@pytest.mark.parametrize('T', [1, 2, 3, 4, 8, 33])      # window remainders 1, 2, 3 of GAE_WIN = 4, one and two exact windows, many
def test_gae_is_the_restatement_and_the_examples_loop_bit_for_bit(T):
    import torch
    rewards, values, v_last, live, nv, carry = gae_case(T)
    gamma, lam = 0.99, 0.95
    for use_nv in (False, True):
        for use_carry in (False, True):
            want = ppo.gae_reference(rewards, values, v_last, live, gamma, lam, nv if use_nv else None, carry if use_carry else None)
            for n in SIZES:
                cut = lambda x: None if x is None else gpu(x[..., :n])
                adv, ret = ppo.gae(cut(rewards), cut(values), cut(v_last), cut(live), gamma, lam, cut(nv if use_nv else None),
                                   cut(carry if use_carry else None))
                assert same(adv.numpy(), want[0][:, :n]) and same(ret.numpy(), want[1][:, :n]), (n, use_nv, use_carry)
    assert (carry != live).any() and (live[0] == 0).any() and (live[T - 1] == 0).any()
    # the default form is the torch loop of examples/ppo_env_loop.py run on the device
    for g, l in ((0.99, 0.95), (0.9, 0.8), (0.997, 0.3)):
        loop = example_loop(rewards, values, v_last, live, g, l, device='cuda')
        adv, ret = ppo.gae(gpu(rewards), values, v_last, live, g, l)
        assert same(adv.numpy(), loop[0]) and same(ret.numpy(), loop[1]), (g, l)
    # ret NULL is not written, and nothing beyond T * n; a NaN reward poisons its own env only
    n = 65
    poisoned = rewards[:, :n].copy()
    poisoned[T - 1, 7] = np.nan
    bufs = dict(rewards=gpu(poisoned), values=gpu(values[:, :n]), v_last=gpu(v_last[:n]), nonterminal=gpu(live[:, :n]))
    adv, ret = torch.full((T * n + 1,), SENTINEL, device='cuda'), torch.full((T * n + 1,), SENTINEL, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    ppo._call(pl._capi.hip_api(), 'eb_gae', C.byref(ppo._gae_args(stream, T, n, gamma, lam, adv=adv, **bufs)))
    torch.cuda.synchronize()
    got = adv.cpu().numpy()
    assert bool((ret == SENTINEL).all()) and got[-1] == SENTINEL
    want = ppo.gae_reference(poisoned, values[:, :n], v_last[:n], live[:, :n], gamma, lam)[0]
    assert same(got[:-1].reshape(T, n), want)
    assert np.isnan(want[T - 1, 7]) and np.isfinite(np.delete(want, 7, axis=1)).all()
    ppo._call(pl._capi.hip_api(), 'eb_gae', C.byref(ppo._gae_args(stream, T, n, gamma, lam, adv=adv, ret=ret, **bufs)))
    torch.cuda.synchronize()
    assert float(ret[-1]) == SENTINEL and same(ret.cpu().numpy()[:-1].reshape(T, n), want + values[:, :n])


# ---- 6: the autograd node against the float64 torch twin --------------------------------------------------------------------------------
def twin(layers, obs, actions, logp_old, adv, adv_norm, hact, oact, scale, action_range, clip, ent_coef, upstream):
    """float64: _policy_cases.torch_twin's layers under the expression of examples/ppo_env_loop.py -> (loss, g_obs, g_params) for
    upstream * loss"""
    import torch
    from torch import distributions as D
    acts = {'linear': lambda x: x, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh}
    params = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for pair in layers for a in pair]
    x0 = torch.tensor(np.asarray(obs, np.float64), requires_grad=True)
    x = x0 if scale is None else x0 * torch.tensor(np.asarray(scale, np.float64))
    for L in range(len(layers)):
        x = acts[oact if L == len(layers) - 1 else hact](x @ params[2 * L] + params[2 * L + 1])
    act_dim = x.shape[1] // 2
    dist = D.Independent(D.Normal(x[:, :act_dim], x[:, act_dim:].exp()), 1)
    if action_range is not None:
        dist = D.TransformedDistribution(dist, [D.transforms.TanhTransform(), D.transforms.AffineTransform(0.0, float(action_range))])
    logp = dist.log_prob(torch.tensor(np.asarray(actions, np.float64)))
    a = (torch.tensor(np.asarray(adv, np.float64)) - float(adv_norm[0])) * float(adv_norm[1])
    ratio = (logp - torch.tensor(np.asarray(logp_old, np.float64))).exp()
    policy_loss = -torch.min(ratio * a, ratio.clamp(1.0 - clip, 1.0 + clip) * a).mean()
    entropy = (x[:, act_dim:] + 0.5 * math.log(2.0 * math.pi * math.e)).sum(1).mean()
    loss = policy_loss - ent_coef * entropy
    (upstream * loss).backward()
    return float(loss.detach()), x0.grad.numpy(), [p.grad.numpy() for p in params]


def restatement32(layers, obs, actions, logp_old, adv, adv_norm, hact, oact, scale, action_range, clip, ent_coef, upstream):
    """the same in float32, from the two NumPy restatements"""
    logits = mlp_backward_reference(layers, obs, np.zeros((len(obs), layers[-1][0].shape[1]), np.float32), hact, oact, scale, 0)[0]
    out = ppo.ppo_reference(logits, actions, logp_old, adv, action_range, clip, ent_coef, adv_norm=adv_norm)
    _, g_obs, g_params = mlp_backward_reference(layers, obs, out['g_logits'] * np.float32(upstream), hact, oact, scale, 0)
    return out['loss'], g_obs, g_params


def bound_failures(got, r32, r64, what):
    """tests/test_gpu_policy_logp.py's rule (tests/test_gpu_policy_grad.py's bar for eb_mlp_backward against its twin): per column of a
    [n, .] output and over a whole parameter tensor or scalar, |got - ref64| <= 4 E + 2^-20 max |ref64| with E = max |ref32 - ref64|"""
    tensors = [('loss', np.float64(got[0]), np.float64(r32[0]), np.float64(r64[0]), None), ('g_obs', got[1], r32[1], r64[1], 0)]
    tensors += [('g_params[%d]' % k, got[2][k], r32[2][k], r64[2][k], None) for k in range(len(r64[2]))]
    failures = []
    for name, a, b32, b64, axis in tensors:
        E = np.abs(np.asarray(b32, np.float64) - b64).max(axis)
        tol = 4.0 * E + 2.0 ** -20 * np.abs(b64).max(axis)
        ratio = float((np.abs(np.asarray(a, np.float64) - b64).max(axis) / np.maximum(tol, 1e-300)).max())
        print('%s %s: error / tolerance %.3f' % (what, name, ratio))
        if not ratio <= 1.0:
            failures.append((what, name, ratio))
    return failures


def test_policy_loss_on_a_trainable_net_against_the_float64_twin():
    import torch
    from env_build_amd.policy_grad import TrainableMLPNet
    cfg = (41, 2, 100, 4, 'elu', 'linear')
    net, layers, scale = make_net(cfg, True, TrainableMLPNet)
    # the output layer's weights times 0.4: the logits of the CPU float32 test (means of a few tenths, log-std inside [-2, 1])
    layers[-1] = ((layers[-1][0] * np.float32(0.4)).astype(np.float32), layers[-1][1])
    net.set_weights([a for pair in layers for a in pair])
    params = net.parameters()
    rng = np.random.default_rng(12)
    n = 200
    obs = rng.standard_normal((n, 41)).astype(np.float32)
    eps = rng.standard_normal((n, 2)).astype(np.float32)
    adv = rng.standard_normal(n).astype(np.float32)
    adv_norm = np.array([0.05, 1.3], np.float32)
    logits32 = mlp_backward_reference(layers, obs, np.zeros((n, 4), np.float32), 'elu', 'linear', scale, 0)[0]
    # a condition on the inputs: the twin has no clamp, so no action may sit on the range (|x| stays where tanh_det is below 1)
    pre = logits32[:, :2].astype(np.float64) + np.exp(logits32[:, 2:].astype(np.float64)) * eps
    assert np.abs(pre).max() <= 6.0 and logits32[:, 2:].min() >= -2.0
    clip = 0.2
    targets = np.array([0.6, 0.95, 1.5])[np.arange(n) % 3]         # below lo, inside, above hi: far from the two edges
    failures = []
    # a secondary guard: ppo.py never touches the logp family's binding, so this counter can only see a regression that routes the
    # backward through policy_logp._call.  The check proper is the node's structure below: what it saved, and that the saved cotangent
    # is the forward launch's g_logits
    vjp_calls = []
    fns = pl.bind(net.api)
    real_vjp = fns['eb_policy_logp_vjp']
    fns['eb_policy_logp_vjp'] = lambda *a: vjp_calls.append(1) or real_vjp(*a)
    try:
        for ar in RANGES:
            actions = ps.policy_sample_reference(logits32, eps, ar)[0]          # what the sampler draws from this network with N(0, 1) noise
            logp32 = pl.policy_logp_reference(logits32, actions, ar)[0]
            logp_old = (logp32.astype(np.float64) - np.log(targets)).astype(np.float32)
            for ent_coef in (0.0, 1e-3):
                for upstream in (1.0, 0.5):
                    x = torch.from_numpy(obs).cuda().requires_grad_(True)
                    for p in params:
                        p.grad = None
                    loss, rows = ppo.policy_loss(net, x, actions, logp_old, adv, ar, clip, ent_coef, adv_norm)
                    assert loss.requires_grad and loss.dim() == 0 and type(loss.grad_fn).__name__ == '_PolicyLossBackward'
                    assert set(rows) == {'logp', 'ratio', 'surr', 'ent'} and not any(t.requires_grad for t in rows.values())
                    assert all(t.shape == (n,) for t in rows.values())
                    r = rows['ratio'].cpu().numpy()
                    assert (r < 0.7).sum() > 50 and (r > 1.35).sum() > 50 and ((r > 0.9) & (r < 1.1)).sum() > 50
                    (loss * upstream).backward()
                    got = (float(loss.detach()), x.grad.cpu().numpy(), [p.grad.cpu().numpy() for p in params])
                    rest = (layers, obs, actions, logp_old, adv, adv_norm, 'elu', 'linear', scale, ar, clip, ent_coef, upstream)
                    failures += bound_failures(got, restatement32(*rest), twin(*rest), 'range %r, ent_coef %g, upstream %g:' % (ar, ent_coef, upstream))
    finally:
        fns['eb_policy_logp_vjp'] = real_vjp
    assert not failures, failures
    assert not vjp_calls                                             # backward is eb_mlp_backward alone: g_logits left the forward launch
    # the node holds the observations and the finished cotangent, nothing of the reverse pass of logp
    actions = ps.policy_sample_reference(logits32, eps, 1.0)[0]
    logp_old = host(pl.log_prob_actions(net, obs, actions, 1.0))['logp']
    loss, rows = ppo.policy_loss(net, obs, actions, logp_old, adv, 1.0, clip, 1e-3, adv_norm)
    assert [tuple(t.shape) for t in loss.grad_fn.saved_tensors] == [(n, 41), (n, 4)]
    assert bool((rows['ratio'] == 1.0).all())
    ref = host(ppo.surrogate(net, obs, actions, logp_old, adv, 1.0, clip, 1e-3, adv_norm, want=('surr', 'ent', 'g_logits')))
    assert same(rows['logp'].cpu().numpy(), ref['logp']) and same(rows['surr'].cpu().numpy(), ref['surr'])
    assert same(loss.grad_fn.saved_tensors[1].cpu().numpy(), ref['g_logits'])
    # weights modified between forward and backward: refused, as log_prob does
    opt = torch.optim.SGD(params, lr=1e-3)
    for p in params:
        p.grad = None
    loss.backward()
    opt.step()
    loss2, _ = ppo.policy_loss(net, obs, actions, logp_old, adv, 1.0, clip, 1e-3, adv_norm)
    opt.step()
    with pytest.raises(RuntimeError, match='modified in place'):
        loss2.backward()
    torch.cuda.synchronize()


# ---- 7: streams and capture: tests/test_gpu_capture.py's obligations, for entries whose stream is a field ---------------------------------
def capture_cases():
    """name -> (run(raw_stream), outputs): each working entry as a raw C call on preallocated buffers"""
    import torch
    cfg = (41, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True)
    rng = np.random.default_rng(6)
    n, T = 130, 5
    x, a = gpu(rng.standard_normal((n, 41))), gpu(rng.uniform(-1.0, 1.0, (n, 2)))
    y = net.call(x).t.clone()
    lo = pl.log_prob_actions(net, x, a, 0.5)['logp'].t + gpu(rng.uniform(-0.5, 0.5, n))
    ad, an = gpu(rng.standard_normal(n)), gpu(np.array([0.1, 1.25]))
    g_in = dict(rewards=gpu(rng.standard_normal((T, n))), values=gpu(rng.standard_normal((T, n))), v_last=gpu(rng.standard_normal(n)),
                nonterminal=gpu(rng.uniform(size=(T, n)) > 0.2))
    api, handle = net.api, net._handle
    new = lambda *shape: torch.full(shape, SENTINEL, device='cuda')
    rows = lambda: dict(logp=new(n), ratio=new(n), surr=new(n), ent=new(n), g_logits=new(n, 4), z_out=new(n, 2))
    fused, alone, adv = dict(rows(), logits_out=new(n, 4)), rows(), dict(adv=new(T, n), ret=new(T, n))
    ins = dict(actions=a, logp_old=lo, adv=ad, adv_norm=an)
    cases = {
        'eb_ppo_surrogate': (lambda s: ppo._call(api, 'eb_ppo_surrogate', handle, C.byref(raw_args(s, n, 0, 0.5, obs=x, **ins, **fused))), fused),
        'eb_ppo_surrogate_from_logits': (
            lambda s: ppo._call(api, 'eb_ppo_surrogate_from_logits', C.byref(raw_args(s, n, 4, 0.5, logits=y, **ins, **alone))), alone),
        'eb_gae': (lambda s: ppo._call(api, 'eb_gae', C.byref(ppo._gae_args(s, T, n, 0.99, 0.95, **g_in, **adv))), adv),
    }
    return net, cases


def test_side_stream_capture_and_replay_for_the_three_entries():
    import torch
    net, cases = capture_cases()
    side = side_stream()

    def snap(outs):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in outs.items()}

    def poison(outs):
        for t in outs.values():
            t.fill_(SENTINEL)
        torch.cuda.synchronize()

    for name, (run, outs) in cases.items():
        poison(outs)
        run(None)                                                   # the null stream
        want = snap(outs)
        assert all((v != SENTINEL).any() for v in want.values()), name
        poison(outs)
        run(side.cuda_stream)                                       # the side stream, eagerly
        got = snap(outs)
        for k in want:
            assert same(got[k], want[k]), '%s on a side stream: %s' % (name, k)
        poison(outs)
        cap = capture(side, run, name)
        try:
            for k, v in snap(outs).items():
                assert (v == SENTINEL).all(), '%s ran under capture: %s' % (name, k)
            nodes = cap.node_types()
            print('%s: %s' % (name, dict(nodes)))
            assert dict(nodes) == {'kernel': 1} and cap.is_chain(), (name, dict(nodes))
            for rep in (1, 2):
                poison(outs)
                cap.replay()
                got = snap(outs)
                for k in want:
                    assert same(got[k], want[k]), '%s replay %d: %s' % (name, rep, k)
        finally:
            cap.close()


# ---- 8: the example ------------------------------------------------------------------------------------------------------------------------
def test_ppo_fused_loop_example_runs():
    spec = importlib.util.spec_from_file_location('ppo_fused_loop', os.path.join(ROOT, 'examples', 'ppo_fused_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(n_env=256, steps=8, epochs=1, minibatches=2, num_hidden_units=64, keep_buffers=True)
    for k in ('policy_loss', 'value_loss', 'entropy', 'clip_fraction', 'approx_kl'):
        assert np.isfinite(out[k]), (k, out[k])
    assert out['policy_delta'] > 0 and out['value_delta'] > 0 and out['steps_per_s'] > 0
    # logp_old comes from eb_policy_logp on the same weights, and the surrogate calls its row function
    assert out['ratio_first'].shape == (256 * 8 // 2,) and (out['ratio_first'] == 1.0).all()
    # its advantages are ppo_env_loop.py's expression on the same buffers
    b = {k: v.cpu().numpy() for k, v in out['buffers'].items()}
    loop = example_loop(b['rewards'], b['values'], b['v_last'], b['nonterminal'], 0.99, 0.95, device='cuda')
    assert same(b['adv'], loop[0]) and same(b['ret'], loop[1]) and np.isfinite(b['adv']).all()
