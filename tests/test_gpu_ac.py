"""GPU (-m gpu): the shared-trunk actor-critic family (include/envbuild_ac.h, env_build_amd.ac).  Every yardstick is code that was there
before it — eb_ppo_surrogate_from_logits + eb_value_loss(stride = W) and eb_policy_sample_from_logits on dense copies, eb_mlp_forward on
the split networks, the minibatch chain issued by hand from the existing entries, collect.Collector on the split networks, torch in
float64 — never the new kernels.  Bit for bit unless a bar is named."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from env_build_amd import _capi, ac, collect, ctl, epoch, ppo, train
from env_build_amd import policy_sample as ps
from tests import _ac as T
from tests._capture import Captured, capture, side_stream
from tests._helpers import ROOT

pytestmark = pytest.mark.gpu
same = T.same


def check(rc):
    ac.ac_api().check(rc)


def place(a):
    """a host array on the device in the middle of a sentinel allocation, at an odd float offset"""
    out = T.Out(*np.shape(a))
    out.t.copy_(T.gpu(a))
    return out


def sync():
    import torch
    torch.cuda.synchronize()


# ---- 1: eb_ac_loss ------------------------------------------------------------------------------------------------------------------------------
LOSS_OUTPUTS = ('logp', 'ratio', 'surr', 'ent', 'vloss', 'g_y', 'z_out')


class LossCase(object):
    """the rows of T.loss_case on the device, and both routes on them"""

    def __init__(self, n, act_dim, action_range):
        self.n, self.A, self.W, self.ar = n, act_dim, 2 * act_dim + 1, action_range
        self.host = T.loss_case(n, act_dim, action_range)
        self.dev = {k: place(self.host[k]) for k in ('y', 'actions', 'logp_old', 'adv', 'ret', 'v_old')}
        self.dense = place(np.ascontiguousarray(self.host['y'][:, :2 * act_dim]))          # the copy the existing entry reads
        self.norm = place(np.array(T.ADV_NORM, np.float32))
        sync()

    def shapes(self):
        n, A, W = self.n, self.A, self.W
        return dict(logp=(n,), ratio=(n,), surr=(n,), ent=(n,), vloss=(n,), g_y=(n, W), z_out=(n, A))

    def ours(self, clip, with_norm, with_v_old, skip=(), stream=None, outs=None):
        d = self.dev
        outs = outs or {k: T.Out(*s) for k, s in self.shapes().items()}
        a = ac.EbAcLossArgs(n=self.n, act_dim=self.A, y=d['y'].ptr(), actions=d['actions'].ptr(), logp_old=d['logp_old'].ptr(), adv=d['adv'].ptr(),
                            adv_norm=self.norm.ptr() if with_norm else None, ret=d['ret'].ptr(), v_old=d['v_old'].ptr() if with_v_old else None,
                            action_range=self.ar, clip=clip, ent_coef=T.ENT_COEF, scale=1.0 / self.n, clip_v=T.CLIP_V, v_scale=T.VF_COEF / self.n,
                            stream=stream, **{k: outs[k].ptr() for k in LOSS_OUTPUTS if k not in skip})
        check(ac.ac_api().loss(C.byref(a)))
        return outs

    def theirs(self, clip, with_norm, with_v_old):
        """eb_ppo_surrogate_from_logits on the dense copy and eb_value_loss on column 2A with stride W"""
        d, n, A, W = self.dev, self.n, self.A, self.W
        outs = dict(logp=T.Out(n), ratio=T.Out(n), surr=T.Out(n), ent=T.Out(n), vloss=T.Out(n), g_logits=T.Out(n, 2 * A), g_values=T.Out(n, W),
                    z_out=T.Out(n, A))
        api = _capi.hip_api()
        a = ppo.EbPpoArgs(n=n, out_dim=2 * A, logits=self.dense.ptr(), actions=d['actions'].ptr(), logp_old=d['logp_old'].ptr(), adv=d['adv'].ptr(),
                          adv_norm=self.norm.ptr() if with_norm else None, action_range=self.ar, clip=clip, ent_coef=T.ENT_COEF, scale=1.0 / n,
                          logp=outs['logp'].ptr(), ratio=outs['ratio'].ptr(), surr=outs['surr'].ptr(), ent=outs['ent'].ptr(),
                          g_logits=outs['g_logits'].ptr(), z_out=outs['z_out'].ptr())
        api.check(ppo.bind(api)['eb_ppo_surrogate_from_logits'](C.byref(a)))
        tr = train.train_api()
        v = train.EbValueLossArgs(n=n, stride=W, values=d['y'].ptr() + 8 * A, ret=d['ret'].ptr(), v_old=d['v_old'].ptr() if with_v_old else None,
                                  clip_v=T.CLIP_V if with_v_old else 0.0, scale=T.VF_COEF / n, loss=outs['vloss'].ptr(),
                                  g_values=outs['g_values'].ptr() + 8 * A)
        tr.check(tr.value_loss(C.byref(v)))
        return outs


def compare_loss(case, got, want, skip=()):
    sync()
    A2 = 2 * case.A
    g = {k: o.host() for k, o in got.items()}
    w = {k: o.host() for k, o in want.items()}
    assert all(ok for _, ok in g.values()), [k for k, (_, ok) in g.items() if not ok]       # the sentinels around every output
    assert all(ok for _, ok in w.values())
    for k in ('logp', 'ratio', 'surr', 'ent', 'vloss', 'z_out'):
        if k in skip:
            assert (g[k][0] == T.SENTINEL).all(), k
        else:
            assert same(g[k][0], w[k][0]), k
    if 'g_y' in skip:
        assert (g['g_y'][0] == T.SENTINEL).all()
    else:
        assert same(g['g_y'][0][:, :A2], w['g_logits'][0]) and same(g['g_y'][0][:, A2], w['g_values'][0][:, A2])
        assert not (g['g_y'][0] == T.SENTINEL).any()                                      # every column written
    return g


@pytest.mark.parametrize('action_range', T.RANGES)
@pytest.mark.parametrize('act_dim', T.ACT_DIMS)
@pytest.mark.parametrize('n', T.SIZES)
def test_ac_loss_equals_the_surrogate_and_the_value_loss_on_copies(n, act_dim, action_range):
    case = LossCase(n, act_dim, action_range)
    for clip in (T.CLIP, 0.0):
        for with_norm in (True, False):
            for with_v_old in (True, False):
                ref = T.loss_reference(case.host, action_range, clip, with_norm, with_v_old)
                if n >= 63:                                       # a single row is one branch; from 63 rows on every branch has its rows
                    missing = T.every_branch_is_taken(case.host, ref, clip, with_v_old)
                    assert not missing, (missing, clip, with_norm, with_v_old)
                g = compare_loss(case, case.ours(clip, with_norm, with_v_old), case.theirs(clip, with_norm, with_v_old))
                if n >= 63:                                       # the NaN rows poison themselves only
                    gy = g['g_y'][0]
                    bad = np.isnan(gy[:, :2 * act_dim]).any(axis=1)
                    assert sorted(np.flatnonzero(bad)) == [T.NAN_LOGIT_ROW, T.NAN_OLD_ROW]
                    assert list(np.flatnonzero(np.isnan(gy[:, 2 * act_dim]))) == [T.NAN_VALUE_ROW]
                    assert list(np.flatnonzero(np.isnan(g['vloss'][0]))) == [T.NAN_VALUE_ROW]
    # each nullable output NULL in turn: the others are the same bits, its buffer keeps its sentinel
    want = case.theirs(T.CLIP, True, True)
    for k in LOSS_OUTPUTS[1:]:
        compare_loss(case, case.ours(T.CLIP, True, True, skip=(k,)), want, skip=(k,))


def test_ac_loss_refuses_on_the_device_without_writing():
    case = LossCase(65, 2, 1.0)
    outs = {k: T.Out(*s) for k, s in case.shapes().items()}
    for kw in (dict(clip=-1.0), dict(act_dim=16), dict(scale=float('nan'))):
        a = ac.EbAcLossArgs(n=65, act_dim=2, y=case.dev['y'].ptr(), actions=case.dev['actions'].ptr(), logp_old=case.dev['logp_old'].ptr(),
                            adv=case.dev['adv'].ptr(), ret=case.dev['ret'].ptr(), action_range=1.0, clip=0.2, scale=1.0, v_scale=1.0,
                            **{k: outs[k].ptr() for k in LOSS_OUTPUTS})
        for k, v in kw.items():
            setattr(a, k, v)
        with pytest.raises(ValueError, match='eb_ac_loss'):
            check(ac.ac_api().loss(C.byref(a)))
    sync()
    assert all((o.host()[0] == T.SENTINEL).all() for o in outs.values())


# ---- 2: eb_ac_sample ----------------------------------------------------------------------------------------------------------------------------
class SampleCase(object):
    def __init__(self, n, act_dim, action_range):
        self.n, self.A, self.W, self.ar = n, act_dim, 2 * act_dim + 1, action_range
        self.host = T.loss_case(n, act_dim, action_range)
        self.y = place(self.host['y'])
        self.dense = place(np.ascontiguousarray(self.host['y'][:, :2 * act_dim]))
        self.eps = place(self.host['eps'])
        self.ids = np.random.default_rng(n).integers(0, 2 ** 31 - 1, n).astype(np.int32)
        import torch
        self.ids_dev = torch.from_numpy(self.ids).cuda()
        sync()

    def outs(self):
        n, A = self.n, self.A
        return dict(actions=T.Out(n, A), logits_out=T.Out(n, 2 * A), values=T.Out(n), logp=T.Out(n), eps_out=T.Out(n, A))

    def ours(self, eps, row_ids, seed, counter, skip=(), stream=None, outs=None):
        outs = outs or self.outs()
        a = ac.EbAcSampleArgs(n=self.n, act_dim=self.A, y=self.y.ptr(), eps=self.eps.ptr() if eps else None,
                              row_ids=self.ids_dev.data_ptr() if row_ids else None, seed=seed, counter=counter, action_range=self.ar, stream=stream,
                              **{k: o.ptr() for k, o in outs.items() if k not in skip})
        check(ac.ac_api().sample(C.byref(a)))
        return outs

    def theirs(self, eps, row_ids, seed, counter):
        n, A = self.n, self.A
        outs = dict(actions=T.Out(n, A), logp=T.Out(n), eps_out=T.Out(n, A))
        api = _capi.hip_api()
        api.check(ps.bind(api)['eb_policy_sample_from_logits'](n, 2 * A, self.dense.ptr(), self.eps.ptr() if eps else None,
                                                              self.ids_dev.data_ptr() if row_ids else None, seed, counter, self.ar,
                                                              outs['actions'].ptr(), outs['logp'].ptr(), outs['eps_out'].ptr(), None))
        return outs


@pytest.mark.parametrize('action_range', T.RANGES)
@pytest.mark.parametrize('act_dim', T.ACT_DIMS)
@pytest.mark.parametrize('n', T.SIZES)
def test_ac_sample_equals_the_sampling_row_on_the_dense_copy(n, act_dim, action_range):
    case = SampleCase(n, act_dim, action_range)
    y = case.host['y']
    drawn = {}
    for eps, row_ids in ((False, False), (True, False), (False, True)):
        got, want = case.ours(eps, row_ids, 7, 3), case.theirs(eps, row_ids, 7, 3)
        sync()
        g = {k: o.host() for k, o in got.items()}
        assert all(ok for _, ok in g.values()) and all(o.host()[1] for o in want.values())
        for k in ('actions', 'logp', 'eps_out'):
            assert same(g[k][0], want[k].host()[0]), (k, eps, row_ids)
        assert same(g['logits_out'][0], y[:, :2 * act_dim]) and same(g['values'][0], y[:, 2 * act_dim])
        drawn[eps, row_ids] = g['eps_out'][0]
    assert same(drawn[True, False], case.host['eps']) and not same(drawn[False, False], drawn[False, True])
    assert same(drawn[False, False], ps.policy_noise_reference(np.arange(n), act_dim, 7, 3))
    assert same(drawn[False, True], ps.policy_noise_reference(case.ids, act_dim, 7, 3))
    # another counter: other noise, the same split
    other = case.ours(False, False, 7, 4)
    sync()
    assert not same(other['eps_out'].host()[0], drawn[False, False]) and same(other['values'].host()[0], y[:, 2 * act_dim])
    # split only: nothing is drawn; actions, logp and eps_out keep their sentinels
    outs = case.outs()
    a = ac.EbAcSampleArgs(n=n, act_dim=act_dim, y=case.y.ptr(), seed=7, counter=3, action_range=action_range, logits_out=outs['logits_out'].ptr(),
                          values=outs['values'].ptr(), logp=outs['logp'].ptr(), eps_out=outs['eps_out'].ptr())
    check(ac.ac_api().sample(C.byref(a)))
    sync()
    g = {k: o.host() for k, o in outs.items()}
    assert all(ok for _, ok in g.values())
    assert all((g[k][0] == T.SENTINEL).all() for k in ('actions', 'logp', 'eps_out'))
    assert same(g['logits_out'][0], y[:, :2 * act_dim]) and same(g['values'][0], y[:, 2 * act_dim])
    # each nullable output NULL in turn
    base = case.theirs(False, False, 7, 3)
    for k in ('logits_out', 'values', 'logp', 'eps_out'):
        got = case.ours(False, False, 7, 3, skip=(k,))
        sync()
        assert (got[k].host()[0] == T.SENTINEL).all() and same(got['actions'].host()[0], base['actions'].host()[0]), k


# ---- 3: streams and capture -----------------------------------------------------------------------------------------------------------------------
def test_both_entries_on_a_side_stream_and_under_capture():
    side = side_stream()
    loss, sample = LossCase(257, 2, 1.0), SampleCase(257, 2, 1.0)
    state = {}

    def reset():
        state['loss'] = {k: T.Out(*s) for k, s in loss.shapes().items()}
        state['sample'] = sample.outs()
        sync()

    def snap():
        sync()
        return {name + k: o.big.cpu().numpy() for name in ('loss', 'sample') for k, o in state[name].items()}

    entries = (('eb_ac_loss', lambda s: loss.ours(T.CLIP, True, True, stream=s, outs=state['loss'])),
               ('eb_ac_sample', lambda s: sample.ours(False, True, 7, 3, stream=s, outs=state['sample'])))
    for name, run in entries:
        reset()
        untouched = snap()
        run(None)
        want = snap()
        assert T.differing(untouched, want), name
        reset()
        run(side.cuda_stream)
        side.synchronize()
        assert not T.differing(want, snap()), name
        reset()
        cap = capture(side, run, name)
        try:
            assert not T.differing(untouched, snap()), '%s ran under capture' % name
            nodes = dict(cap.node_types())
            print('%s:' % name, nodes)
            assert nodes == {'kernel': 1} and cap.is_chain(), name                        # no memset, no memcpy
            cap.replay()
            side.synchronize()
            assert not T.differing(want, snap()), name
        finally:
            cap.close()


# ---- 4: ac.split ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('units', [64, 128, 256])
def test_split_networks_are_the_shared_networks_columns(units, B):
    import torch
    net = T.make_net((41, 2, units, 5, 'elu', 'linear'))
    policy, value = ac.split(net)
    assert (policy.output_dim, value.output_dim) == (4, 1) and policy.num_hidden_units == value.num_hidden_units == units
    obs = T.gpu(np.random.default_rng(units + B).standard_normal((B, 41)))
    with torch.no_grad():
        y = net.call(obs).cpu().numpy()
    assert y.shape == (B, 5) and np.isfinite(y).all() and np.abs(y).max() > 0.1
    assert same(policy.call(obs).numpy(), y[:, :4]) and same(value.call(obs).numpy(), y[:, 4:])
    # the other consumers of a 2A-wide handle take the split policy: the mode is action_range * tanh(mean)
    assert policy.mode(obs, 1.0).numpy().shape == (B, 2)


# ---- 5: ac.PPOUpdate ----------------------------------------------------------------------------------------------------------------------------------
class HandChain(object):
    """the minibatch of ac.PPOUpdate issued by hand from entries that were there before it: eb_mlp_forward, a dense copy of the logits
    made with torch, eb_ppo_surrogate_from_logits, eb_value_loss(stride = W), eb_mlp_backward and train.Adam"""

    def __init__(self, net, n):
        import torch
        from env_build_amd.dynamics_and_models import _stream
        self._stream = _stream
        self.net = self.policy = self.value = net
        self.n, self.api, dev = n, net.api, net.device
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.mb = train._Buffers(obs=new(n, 41), actions=new(n, 2), logp_old=new(n), adv=new(n), ret=new(n), v_old=new(n), adv_norm=new(2))
        self.rows = train._Buffers(logp=new(n), ratio=new(n), surr=new(n), ent=new(n), vloss=new(n))
        self.y, self.g_y, self.g_logits = new(n, 5), new(n, 5), new(n, 4)
        kw = {k: T.PPO_KW[k] for k in ('lr', 'betas', 'eps', 'max_grad_norm')}
        self.adam = train.Adam([net], **kw)
        net._sync()
        need = C.c_size_t(0)
        self.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
        self.ws, self.need = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value

    def step(self):
        net, api, n, mb, rows = self.net, self.api, self.n, self.mb, self.rows
        net._sync()
        s = self._stream(net.device)
        api.mlp_forward(net._h, n, mb.obs.data_ptr(), self.y.data_ptr(), s)
        dense = self.y[:, :4].contiguous()
        a = ppo._args(s, n, 4, 1.0, T.CLIP, float(np.float32(T.ENT_COEF)), 1.0 / n, logits=dense, actions=mb.actions, logp_old=mb.logp_old, adv=mb.adv,
                      adv_norm=mb.adv_norm, logp=rows.logp, ratio=rows.ratio, surr=rows.surr, ent=rows.ent, g_logits=self.g_logits)
        api.check(ppo.bind(api)['eb_ppo_surrogate_from_logits'](C.byref(a)))
        tr = train.train_api()
        v = train.EbValueLossArgs(n=n, stride=5, values=self.y.data_ptr() + 16, ret=mb.ret.data_ptr(), v_old=mb.v_old.data_ptr(), clip_v=T.CLIP_V,
                                  scale=T.VF_COEF / n, loss=rows.vloss.data_ptr(), g_values=self.g_y.data_ptr() + 16, stream=s)
        tr.check(tr.value_loss(C.byref(v)))
        self.g_y[:, :4].copy_(self.g_logits)
        api.mlp_backward(net._h, n, mb.obs.data_ptr(), self.g_y.data_ptr(), 0, 0.0, self.ws.data_ptr(), self.need, None, None,
                         self.adam.grads[0].data_ptr(), s)
        self.adam.issue()
        self.adam.bump()


@pytest.mark.parametrize('n', [65, 256])
def test_ppo_update_equals_the_chain_issued_by_hand_and_is_eight_kernels(n):
    import torch
    net, twin = T.make_net(), T.make_net()
    data = T.make_data(net, 2 * n, seed=n)
    batches = [slice(0, n), slice(n, 2 * n)]
    upd, hand = ac.PPOUpdate(net, n, **T.PPO_KW), HandChain(twin, n)
    assert type(upd) is ac.PPOUpdate and upd.policy is net and upd.value is net and upd.control is None
    assert isinstance(upd.adam, train.Adam) and not isinstance(upd.adam, ctl.Adam) and float(upd._ppo_args.clip) == float(np.float32(T.CLIP))
    held = []
    for k, rows in enumerate(batches):
        T.fill(upd, data, rows)
        T.fill(hand, data, rows)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_stats()['allocation.all.allocated']
        upd.step()
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == allocated          # no allocation across a step
        hand.step()
        got, want = T.snapshot(upd), T.snapshot(hand)
        assert not T.differing(want, got), (k, T.differing(want, got))
        assert got['state'][0] == k + 1 and net._uploaded == net._flat._version
        held.append(got)
    assert (held[0]['ratio'] == 1.0).all() and not (held[1]['ratio'] == 1.0).all()        # logp_old is eb_policy_logp's on the first weights
    assert not same(held[0]['net'], held[1]['net']) and (held[0]['vloss'] > 0).any()
    # captured: 8 kernel nodes in one chain, nothing else; two replays are the two eager steps
    net2 = T.make_net()
    cap = ac.PPOUpdate(net2, n, **T.PPO_KW)
    T.fill(cap, data, batches[0])
    before = T.snapshot(cap)
    graph = cap.capture(keep_graph=True)
    assert not T.differing(before, T.snapshot(cap)), 'the chain ran under capture'
    seen = Captured(graph, torch.cuda.current_stream(), 'ac.PPOUpdate.step')
    nodes = dict(seen.node_types())
    print('ac.PPOUpdate.step:', nodes)
    assert nodes == {'kernel': 8} and seen.is_chain()                                      # two backwards would be 11 or more
    for k, rows in enumerate(batches):
        T.fill(cap, data, rows)
        version = net2._flat._version
        cap.replay(graph)
        assert net2._flat._version > version and net2._uploaded == net2._flat._version
        got = T.snapshot(cap)
        assert not T.differing(held[k], got), (k, T.differing(held[k], got))
    obs = data['obs'][:7]
    with torch.no_grad():
        assert same(net2.call(obs).cpu().numpy(), net.call(obs).cpu().numpy())             # the handle followed the replays
    torch.cuda.synchronize()
    graph.reset()


def torch_step(params, scale, data, dtype, device):
    """the loss of the autograd route in plain torch at `dtype` on the shared network's six parameter tensors `params` (leaves): the
    network written out, then torch_loss"""
    import torch
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype, device=device)
    x = t(data['obs']) * t(scale)
    for L in range(0, len(params), 2):
        x = x @ params[L] + params[L + 1]
        if L < len(params) - 2:
            x = torch.nn.functional.elu(x)
    return torch_loss(x, data, t)


def torch_loss(y, data, t):
    """TransformedDistribution.log_prob, the clipped surrogate with its entropy bonus and the clipped value loss on column 4 of y"""
    import torch
    from torch import distributions as D
    dist = D.TransformedDistribution(D.Independent(D.Normal(y[:, :2], y[:, 2:4].exp()), 1),
                                     [D.transforms.TanhTransform(), D.transforms.AffineTransform(0.0, 1.0)])
    logp = dist.log_prob(t(data['actions']))
    A = (t(data['adv']) - t(np.float32(T.ADV_NORM[0]))) * t(np.float32(T.ADV_NORM[1]))
    ratio = (logp - t(data['logp_old'])).exp()
    surr = torch.min(ratio * A, ratio.clamp(1.0 - T.CLIP, 1.0 + T.CLIP) * A)
    entropy = (y[:, 2:4] + 0.5 * math.log(2.0 * math.pi * math.e)).sum(1).mean()
    v, ret, v_old = y[:, 4], t(data['ret']), t(data['v_old'])
    vloss = (0.5 * torch.max((v - ret) ** 2, (v_old + (v - v_old).clamp(-T.CLIP_V, T.CLIP_V) - ret) ** 2)).mean()
    return -surr.mean() - float(np.float32(T.ENT_COEF)) * entropy + T.VF_COEF * vloss


def test_ppo_update_matches_the_autograd_route_under_the_4e_rule():
    """One step from equal weights at 256 rows.  The route: the shared TrainableMLPNet on the autograd graph, the loss in torch float32
    on the device, clip_grad_norm_ and torch.optim.Adam.  E, per parameter tensor, is that route's distance from its float64 twin (plain
    torch on the host); ac.PPOUpdate is held to 4 E + 2^-20 of the tensor's maximum — tests/test_gpu_train.py case (5)'s rule.  logp_old
    is off the present logp by up to +-0.3, so rows sit on both sides of the clip interval.
    Measured: see DESIGN.md §28."""
    import torch
    n = 256
    net = T.make_net()
    data = T.make_data(net, n, seed=9, shift=0.3)
    host = {k: v.cpu().numpy() for k, v in data.items()}
    upd = ac.PPOUpdate(net, n, **T.PPO_KW)
    T.fill(upd, data)
    upd.step()
    torch.cuda.synchronize()
    ratio = upd.rows.ratio.cpu().numpy()
    assert (ratio < 0.8).sum() > 20 and (ratio > 1.2).sum() > 20 and float(upd.adam.state.coef.cpu()[0]) < 1.0
    ours = [p.detach().cpu().numpy().astype(np.float64) for p in net.parameters()]
    # the autograd route, float32 on the device
    net3 = T.make_net()
    params = net3.parameters()
    opt = torch.optim.Adam(params, lr=T.LR, betas=T.BETAS, eps=T.EPS)
    t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device='cuda')
    torch_loss(net3(data['obs']), host, t32).backward()
    torch.nn.utils.clip_grad_norm_(params, T.PPO_KW['max_grad_norm'])
    opt.step()
    torch.cuda.synchronize()
    route = [p.detach().cpu().numpy().astype(np.float64) for p in params]
    # the float64 twin, plain torch on the host
    layers, scale = T.net_layers()
    start = [np.asarray(a, np.float64) for pair in layers for a in pair]
    leaves = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in start]
    opt64 = torch.optim.Adam(leaves, lr=T.LR, betas=T.BETAS, eps=T.EPS)
    torch_step(leaves, scale, host, torch.float64, 'cpu').backward()
    torch.nn.utils.clip_grad_norm_(leaves, T.PPO_KW['max_grad_norm'])
    opt64.step()
    twin = [p.detach().numpy() for p in leaves]
    worst = 0.0
    for k, (mine, theirs, want, was) in enumerate(zip(ours, route, twin, start)):
        E = np.abs(theirs - want).max()
        err = np.abs(mine - want).max()
        moved = np.abs(want - was).max()
        print('parameter %d: moved %.3g, error %.3g, E %.3g, ratio %.2f' % (k, moved, err, E, err / max(E, 1e-30)))
        assert moved > 0.1 * T.LR                                      # the step is there: one Adam step moves a weight by about lr
        assert err <= 4.0 * E + 2.0 ** -20 * np.abs(want).max(), 'parameter %d: error %.3g, E %.3g' % (k, err, E)
        worst = max(worst, err / max(E, 1e-30))
    print('worst ratio to E: %.2f' % worst)


# ---- 6: the drivers -----------------------------------------------------------------------------------------------------------------------------------
ROWS, EPOCHS, MINIBATCHES, SEED = 64, 2, 2, 11
SLOTS = EPOCHS * MINIBATCHES
N = MINIBATCHES * ROWS + 3


def epochs_case(controlled, **control_kw):
    """(loop, update) on the shared network and 131 rows, 2 epochs x 2 minibatches of 64 rows under the keyed shuffle"""
    net = T.make_net()
    data = T.make_data(net, N, seed=6)
    upd = ac.PPOUpdate(net, ROWS, **dict(T.PPO_KW, **control_kw))
    if controlled:
        return ctl.PPOEpochs(upd, data, EPOCHS, MINIBATCHES, seed=SEED), upd
    return epoch.PPOEpochs(upd, data, EPOCHS, MINIBATCHES, seed=SEED), upd


def moved(upd):
    snap = T.snapshot(upd)
    return {k: snap[k] for k in ('net', 'm', 'v', 'state')}


def nodes_of(loop, what):
    import torch
    graph = loop.capture(keep_graph=True)
    seen = Captured(graph, torch.cuda.current_stream(), what)
    nodes, chain = dict(seen.node_types()), seen.is_chain()
    print('%s:' % what, nodes)
    return graph, nodes, chain


def test_the_epoch_drivers_take_the_shared_update_unchanged():
    import torch
    # epoch.PPOEpochs: 3 + 10 * 4 kernels; two replays are two eager iterations
    loop, upd = epochs_case(False)
    assert type(upd) is ac.PPOUpdate
    want = []
    for _ in range(2):
        loop.step()
        want.append((T.snapshot(upd), loop.log()))
    assert want[0][0]['state'][0] == SLOTS and want[0][1]['approx_kl'][0, 0] == 0.0
    loop, upd = epochs_case(False)
    before = T.snapshot(upd)
    graph, nodes, chain = nodes_of(loop, 'epoch.PPOEpochs over ac.PPOUpdate')
    assert not T.differing(before, T.snapshot(upd)) and nodes == {'kernel': 3 + 10 * SLOTS} and chain
    for i in range(2):
        loop.replay(graph)
        got, log = T.snapshot(upd), loop.log()
        assert not T.differing(want[i][0], got) and all(np.array_equal(log[k], want[i][1][k], equal_nan=True) for k in log), i
    torch.cuda.synchronize()
    graph.reset()
    plain = want
    # ctl.PPOEpochs without a table or a limit: 4 + 10 * 4 kernels and the plain run's weights
    loop, upd = epochs_case(True, control=ctl.UpdateControl('cuda'))
    assert type(upd) is ac.ControlledPPOUpdate and isinstance(upd.adam, ctl.Adam)
    graph, nodes, chain = nodes_of(loop, 'ctl.PPOEpochs over ac.PPOUpdate')
    assert nodes == {'kernel': 4 + 10 * SLOTS} and chain
    loop.replay(graph)
    assert not T.differing(plain[0][0], T.snapshot(upd)) and (loop.log()['applied'] == 1).all()
    torch.cuda.synchronize()
    graph.reset()
    # the table [1, 0.5, 0]: three replays equal three eager iterations; the first is the plain run's, the third moves no weight
    loop, upd = epochs_case(True, lr_table=[1.0, 0.5, 0.0])
    eager = []
    for _ in range(3):
        loop.step()
        eager.append((T.snapshot(upd), loop.log()))
    assert not T.differing(plain[0][0], eager[0][0]) and T.differing(plain[1][0], eager[1][0])
    assert same(eager[1][0]['net'], eager[2][0]['net']) and not same(eager[1][0]['m'], eager[2][0]['m'])
    assert [float(e[1]['lr_scale']) for e in eager] == [1.0, 0.5, 0.0]
    loop, upd = epochs_case(True, lr_table=[1.0, 0.5, 0.0])
    graph, nodes, chain = nodes_of(loop, 'ctl.PPOEpochs over ac.PPOUpdate, table')
    assert nodes == {'kernel': 4 + 10 * SLOTS} and chain and upd.control.host()['iteration'] == 0
    for i in range(3):
        loop.replay(graph)
        got, log = T.snapshot(upd), loop.log()
        assert not T.differing(eager[i][0], got), (i, T.differing(eager[i][0], got))
        assert all(np.array_equal(log[k], eager[i][1][k], equal_nan=True) for k in log), i
    torch.cuda.synchronize()
    graph.reset()


def test_a_kl_stop_leaves_the_shared_networks_weights_and_adam_state_untouched():
    import torch
    loop, upd = epochs_case(False)
    loop.step()
    kl = loop.log()['approx_kl'].ravel()
    print('approx_kl per slot of the uncontrolled run:', ' '.join('%+.6e' % x for x in kl))
    assert kl[0] == 0.0
    rising = [j for j in range(1, SLOTS) if kl[j] > kl[:j].max()]
    assert rising, 'no slot of the case has a KL above every earlier one: pick another seed'
    j = rising[0]
    limit = 0.5 * (kl[j] + kl[:j].max())
    # the yardstick: an uncontrolled run whose first j (gather, step) pairs alone were issued
    part, upd_p = epochs_case(False)
    with torch.cuda.device(part.device):
        part.api.check(part.api.adv_stats(C.byref(part._stats)))
        for g in part._gathers[:j]:
            part.api.check(part.api.minibatch_gather(C.byref(g)))
            upd_p.step()
    want = moved(upd_p)
    assert want['state'][0] == j
    applied = np.array([1] * j + [0] * (SLOTS - j)).reshape(EPOCHS, MINIBATCHES)
    loop, upd = epochs_case(True, target_kl=limit, kl_factor=1.0)
    assert type(upd) is ac.ControlledPPOUpdate and upd.control.limit == limit
    graph, nodes, chain = nodes_of(loop, 'ctl.PPOEpochs over ac.PPOUpdate, target_kl')
    assert nodes == {'kernel': 4 + 12 * SLOTS} and chain
    loop.replay(graph)
    got, log = moved(upd), loop.log()
    assert not T.differing(want, got), T.differing(want, got)
    assert log['stopped_at'] == j and np.array_equal(log['applied'], applied)
    assert np.array_equal(log['approx_kl'].ravel()[:j + 1], kl[:j + 1]) and np.isfinite(log['approx_kl']).all()
    torch.cuda.synchronize()
    graph.reset()
    # eagerly, the same
    loop, upd = epochs_case(True, target_kl=limit, kl_factor=1.0)
    loop.step()
    assert not T.differing(want, moved(upd)) and loop.log()['stopped_at'] == j


# ---- 7: ac.Collector ------------------------------------------------------------------------------------------------------------------------------------
GAMMA, LAM, ENV_SEED = 0.99, 0.95, 0


def make_env(limit=5):
    from env_build_amd.endtoend import CrossroadEnd2end
    env = CrossroadEnd2end('left', n_env=65, auto_reset=True, copy_outputs=False, max_episode_steps=limit)
    env.seed(ENV_SEED)
    env.reset()
    env.reset()
    return env


def test_collector_equals_the_two_network_collector_on_the_split_networks():
    import torch
    Tn, B, seed = 5, 65, 11
    env_p, env_c = make_env(), make_env()
    scale = np.array([0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env_p.veh_num, np.float32)
    assert env_p.obs_dim == 41
    net = T.make_net(scale=scale)
    policy, value = ac.split(net)
    parent = collect.Collector(env_p, policy, value, Tn, 1.0, seed=seed)
    col = ac.Collector(env_c, net, Tn, 1.0, seed=seed)
    assert col.policy is net and col.value is net
    host = lambda t: t.detach().cpu().numpy()
    truncated = 0
    for iteration in range(2):
        parent.collect()
        want = parent.finish(GAMMA, LAM)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_stats()['allocation.all.allocated']
        col.collect()
        got = col.finish(GAMMA, LAM)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == allocated, iteration      # no allocation
        torch.cuda.synchronize()
        assert sorted(got) == sorted(want) == ['actions', 'adv', 'logp_old', 'obs', 'ret', 'v_old']
        for k in want:
            assert host(got[k]).tobytes() == host(want[k]).tobytes(), (iteration, k)
        for k in ('logit_buf', 'values', 'v_trunc', 'next_values'):
            assert host(getattr(col, k)).tobytes() == host(getattr(parent, k)).tobytes(), (iteration, k)
        for k in ('trunc_obs', 'trunc_t', 'rew_buf', 'code_buf', 'obs_buf'):
            assert host(col.buf[k]).tobytes() == host(parent.buf[k]).tobytes(), (iteration, k)
        assert same(host(col.y_buf)[..., 4], host(col.values[:Tn])) and np.isfinite(host(got['adv'])).all()
        assert col.episodes() == parent.episodes()
        truncated += int((host(col.buf['trunc_t']) >= 0).sum())
    assert truncated > 0 and col.iteration == 2                       # otherwise the bootstrap rows prove nothing
    # fed to PPOEpochs: the one minibatch of all rows has ratio exactly 1.0 — logp_old is eb_policy_logp's on the same weights
    upd = ac.PPOUpdate(net, Tn * B, **T.PPO_KW)
    loop = epoch.PPOEpochs(upd, col.data, 1, 1, seed=seed)
    loop.step()
    torch.cuda.synchronize()
    assert (host(upd.rows.ratio) == 1.0).all() and np.isfinite(host(upd.rows.vloss)).all()


def test_collector_and_update_refuse_what_they_cannot_run():
    from env_build_amd.policy_grad import TrainableMLPNet
    env = make_env()
    net = T.make_net()
    even = TrainableMLPNet(41, 2, 64, 'elu', 4)
    with pytest.raises(ValueError):
        ac.Collector(env, even, 5, 1.0)
    with pytest.raises(ValueError, match='max_episode_steps'):
        ac.Collector(env, net, 6, 1.0)
    with pytest.raises(TypeError):
        ac.Collector(object(), net, 5, 1.0)
    with pytest.raises(ValueError):
        ac.PPOUpdate(even, 64, 1.0, 0.2)
    with pytest.raises(TypeError):
        ac.PPOUpdate(object(), 64, 1.0, 0.2)
    with pytest.raises(ValueError):
        ac.PPOUpdate(net, 64, 1.0, 0.2, control=ctl.UpdateControl('cuda'), target_kl=0.01)
    with pytest.raises(TypeError):
        ctl.PPOEpochs(ac.PPOUpdate(net, 64, 1.0, 0.2), {}, 1, 1)      # without a control it is no ctl.PPOUpdate


# ---- 8: the example ---------------------------------------------------------------------------------------------------------------------------------------
def test_ppo_shared_loop_example_runs():
    spec = importlib.util.spec_from_file_location('ppo_shared_loop', os.path.join(ROOT, 'examples', 'ppo_shared_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(n_env=256, steps=8, iterations=3, epochs=2, minibatches=2, num_hidden_units=64)
    assert same(res['table'], np.array([1.0, 0.5, 0.0], np.float32)) and res['iterations_begun'] == 3
    taken = 0
    for i, log in enumerate(res['logs']):
        for name in ('policy_loss', 'value_loss', 'entropy', 'clip_fraction', 'approx_kl', 'max_ratio_dev'):
            assert log[name].shape == (2, 2) and np.isfinite(log[name]).all(), (i, name)
        assert (log['nonfinite_rows'] == 0).all() and (log['rows'] == 1024).all() and log['lr_scale'] == res['table'][i]
        taken += int(log['applied'].sum())
    assert res['optimiser_steps'] == taken and res['deltas'][0] > 0.0                      # the net moved
    assert res['logits'].shape == (256, 4) and res['shared'].shape == (256, 5) and res['mode'].shape == (256, 2)
    assert same(res['logits'], res['shared'][:, :4]) and np.isfinite(res['mode']).all()
