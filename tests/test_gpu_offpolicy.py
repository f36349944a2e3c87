"""GPU (-m gpu): the off-policy family on the MI355X, bit for bit against the NumPy restatements of env_build_amd.offpolicy — the ring's
push and sample, the pack, critic, actor, action-gradient and Polyak rows, every entry on a side stream and under capture,
`offpolicy.Collector` against a loop written out in the test, `offpolicy.SAC` against the same chain issued call by call and against a
torch float64 twin under autograd, and the example.  Every buffer of the entry tests is a view into the middle of a larger allocation with
sentinel slack, once 16-byte aligned (slack 4) and once at an odd float offset (slack 3)."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest

from env_build_amd import offpolicy as O
from tests import _offpolicy as T
from tests._capture import Captured, capture, side_stream
from tests._collect import Slack
from tests._helpers import ROOT
from tests._offpolicy import bits
from tests._ppo import gpu

pytestmark = pytest.mark.gpu

S = T.SENTINEL


def word(value=-77):
    """an 8-byte device word in the middle of three -> (the three, the view of the middle one)"""
    import torch
    big = torch.full((3,), value, dtype=torch.int64, device='cuda')
    return big, big[1:2]


def host(t):
    return t.detach().cpu().numpy()


def call(name, a, stream=None):
    api = O.offpolicy_api()
    a.stream = stream
    api.check(getattr(api.lib, name)(C.byref(a)))


# ---- 1: the ring -------------------------------------------------------------------------------------------------------------------------------
PUSH_VARIANTS = (('before', False), ('after', True), ('after', False), ('both', True), ('both', False))


@pytest.mark.parametrize('slack', [4, 3])
@pytest.mark.parametrize('C_', [5, 64, 257])
def test_push_equals_the_restatement(C_, slack):
    """n in {1, 3, 64, 65} (n <= C), start in {0, C - 1, C - n}, D in {1, 41, 137}, A in {1, 2}; on one ring of sentinels the five calls
    one after the other — the before part alone, the after part alone with and without final_obs, both parts with and without — each
    with the codes 0 .. 7 across its rows.  The whole ring is compared after every call, so the slots not written keep their
    sentinels; *fill moves only with the after part."""
    import torch
    for n, D, A in itertools.product((1, 3, 64, 65), (1, 41, 137), (1, 2)):
        if n > C_:
            continue
        for start in sorted({0, C_ - 1, C_ - n}):
            want = T.ring_arrays(C_, D, A, sentinel=True)
            steps = [T.step_arrays(n, D, A, seed=k) for k in range(len(PUSH_VARIANTS))]
            arrays = dict(want)
            for k, st in enumerate(steps):
                arrays.update({'%s%d' % (name, k): a for name, a in st.items()})
            d = Slack(arrays, slack)
            v = d.views
            assert (v['obs'].data_ptr() % 16 == 0) == (slack == 4)
            fill_big, fill = word()
            want_fill = -77
            for k, ((parts, final), st) in enumerate(zip(PUSH_VARIANTS, steps)):
                p = lambda name: v['%s%d' % (name, k)].data_ptr()
                a = O.EbReplayPushArgs(capacity=C_, n=n, start=start, obs_dim=D, act_dim=A, fill_after=min(C_, k + 1), fill=fill.data_ptr(),
                                       **{r: v[r].data_ptr() for r in T.RING})
                kw = {}
                if parts in ('before', 'both'):
                    a.prev_obs, a.action = p('prev_obs'), p('action')
                    kw.update(prev_obs=st['prev_obs'], action=st['action'])
                if parts in ('after', 'both'):
                    a.reward, a.obs_after, a.done_code = p('reward'), p('obs_after'), p('done_code')
                    kw.update(reward=st['reward'], obs_after=st['obs_after'], done_code=st['done_code'])
                    want_fill = min(C_, k + 1)
                    if final:
                        a.final_obs = p('final_obs')
                        kw.update(final_obs=st['final_obs'])
                call('eb_replay_push', a)
                O.push_reference(want, start, **kw)
                torch.cuda.synchronize()
                for r in T.RING:
                    assert bits(host(v[r]), want[r]), (n, D, A, start, parts, final, r)
                assert host(fill_big).tolist() == [-77, want_fill, -77], (n, D, A, start, parts, final)
            have, untouched = d.host()
            assert untouched, (n, D, A, start)
            for k, st in enumerate(steps):
                assert all(bits(have['%s%d' % (name, k)], a) for name, a in st.items())        # the inputs are unchanged
            if n < C_:
                assert (want['rew'] == S).any() and (want['obs'] == S).any()                   # some slot was never written


OUTS = ('obs', 'qin', 'next_obs', 'rew', 'nonterminal', 'index', 'noise_id')


@pytest.mark.parametrize('slack', [4, 3])
@pytest.mark.parametrize('m', [1, 31, 32, 33, 257])
def test_sample_equals_the_restatement(m, slack):
    """f in {0, 1, 2, C}, the keyed route (with and without a device counter) and the explicit route (int32 and int64, with indices out of
    [0, f): NaN rows and -1, nothing dereferenced), all seven outputs and every subset that leaves one out"""
    import torch
    C_, D, A = 67, 41, 2
    ring = T.ring_arrays(C_, D, A, seed=m)
    shapes = dict(obs=(m, D), qin=(m, D + A), next_obs=(m, D), rew=(m,), nonterminal=(m,))
    arrays = dict(ring)
    arrays.update({'out_' + k: np.full(s, S, np.float32) for k, s in shapes.items()})
    arrays.update(out_index=np.full(m, -77, np.int32), out_noise_id=np.full(m, -77, np.int32))
    d = Slack(arrays, slack)
    v = d.views
    fill_big, fill = word()
    counter_big, counter = word(5)
    rng = np.random.default_rng(m)
    subsets = [OUTS] + [tuple(o for o in OUTS if o != left) for left in OUTS]
    for f in (0, 1, 2, C_):
        fill.fill_(f)
        explicit = rng.integers(0, max(f, 1), m).astype(np.int64)
        explicit[::5] = np.array([-1, f, 2 ** 31 - 1, -2 ** 31, f + 1])[np.arange(len(explicit[::5])) % 5]
        explicit64 = explicit.copy()
        explicit64[::7] = 2 ** 40 + 3
        routes = [dict(seed=9, draw=3), dict(seed=9, draw=1, counter=counter), dict(indices=gpu(explicit, np.int32)),
                  dict(indices=gpu(explicit64, np.int64))]
        wants = [O.sample_reference(ring, f, m, 9, 3), O.sample_reference(ring, f, m, 9, 1, base=5),
                 O.sample_reference(ring, f, m, indices=explicit), O.sample_reference(ring, f, m, indices=explicit64)]
        assert bits(wants[0]['index'], O.sample_index_reference(m, f, 9, 3).astype(np.int32))
        for (route, want), outs in itertools.product(zip(routes, wants), subsets):
            for k in OUTS:
                d.big['out_' + k].fill_(d.fill['out_' + k])
            a = O.EbReplaySampleArgs(capacity=C_, m=m, obs_dim=D, act_dim=A, fill=fill.data_ptr(), seed=route.get('seed', 0),
                                     draw=route.get('draw', 0), **{r: v[r].data_ptr() for r in T.RING})
            if 'counter' in route:
                a.counter = counter.data_ptr()
            if 'indices' in route:
                a.indices, a.index_bytes = route['indices'].data_ptr(), route['indices'].element_size()
            for k in outs:
                setattr(a, k + '_out', v['out_' + k].data_ptr())
            call('eb_replay_sample', a)
            have, untouched = d.host()
            assert untouched, (f, outs)
            for k in OUTS:
                if k in outs:
                    w = want[k].view(np.int32) if k == 'noise_id' else want[k]
                    assert bits(have['out_' + k], w), (f, k, sorted(route), outs)
                else:
                    assert (have['out_' + k] == d.fill['out_' + k]).all(), (f, k)
            assert all(bits(have[r], ring[r]) for r in T.RING)
            if 'indices' in route or f == 0:
                bad = want['index'] < 0
                assert bad.any() and np.isnan(want['qin'][bad]).all() and (m < 5 or f == 0 or (~bad).any())
    assert host(fill_big).tolist() == [-77, C_, -77] and host(counter_big).tolist() == [5, 5, 5]


# ---- 2: the rows ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slack', [4, 3])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 257])
def test_pack_and_action_grad_equal_the_restatements(m, slack):
    for D, A in ((41, 2), (1, 1), (137, 16)):
        rng = np.random.default_rng(m + D)
        obs, act = rng.standard_normal((m, D)).astype(np.float32), rng.standard_normal((m, A)).astype(np.float32)
        g1, g2 = rng.standard_normal((m, D + A)).astype(np.float32), rng.standard_normal((m, D + A)).astype(np.float32)
        g1[0, D] = np.nan
        arrays = dict(obs=obs, act=act, g1=g1, g2=g2, ga=np.full((m, A), S, np.float32), ga1=np.full((m, A), S, np.float32))
        arrays.update({k: np.full((m, D + A), S, np.float32) for k in ('q_both', 'q_obs', 'q_act')})
        d = Slack(arrays, slack)
        v = d.views
        for k, (o, a_) in (('q_both', ('obs', 'act')), ('q_obs', ('obs', None)), ('q_act', (None, 'act'))):
            call('eb_q_pack', O.EbQPackArgs(m=m, obs_dim=D, act_dim=A, obs=v[o].data_ptr() if o else None, act=v[a_].data_ptr() if a_ else None,
                                           qin=v[k].data_ptr()))
        call('eb_q_action_grad', O.EbQActionGradArgs(m=m, obs_dim=D, act_dim=A, g_in1=v['g1'].data_ptr(), g_in2=v['g2'].data_ptr(), g_a=v['ga'].data_ptr()))
        call('eb_q_action_grad', O.EbQActionGradArgs(m=m, obs_dim=D, act_dim=A, g_in1=v['g1'].data_ptr(), g_a=v['ga1'].data_ptr()))
        have, untouched = d.host()
        assert untouched
        blank = lambda: np.full((m, D + A), S, np.float32)
        assert bits(have['q_both'], O.q_pack_reference(blank(), obs, act)) and bits(have['q_obs'], O.q_pack_reference(blank(), obs, None))
        assert bits(have['q_act'], O.q_pack_reference(blank(), None, act)) and (have['q_obs'][:, D:] == S).all() and (have['q_act'][:, :D] == S).all()
        assert bits(have['ga'], O.action_grad_reference(g1, g2, A)) and bits(have['ga1'], O.action_grad_reference(g1, None, A))
        assert np.isnan(have['ga'][0, 0]) and np.isfinite(have['ga'].reshape(-1)[1:]).all()
        assert all(bits(have[k], arrays[k]) for k in ('obs', 'act', 'g1', 'g2'))


CRITIC_OUT = ('y', 'loss1', 'loss2', 'g_q1', 'g_q2')
ACTOR_OUT = ('loss', 'g_q1', 'g_q2', 'g_logp')


@pytest.mark.parametrize('slack', [4, 3])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 257, 64 * 256 + 1])
def test_critic_and_actor_equal_the_restatements(m, slack):
    """alpha by value and log_alpha on the device; clean rows, then a NaN, a +inf and a -inf row: they poison only themselves, and through
    S the temperature gradient.  m = 64 * 256 + 1 is one row more than one pass of the actor's 64-block grid."""
    import torch
    clean = T.row_inputs(m, seed=m)
    dirty = [x.copy() for x in clean]
    poisoned = list(range(min(m, 3)))
    for row, bad in zip(poisoned, (np.nan, np.inf, -np.inf)):
        dirty[row % 2][row] = bad                                         # q1t / q2t of the critic, q1 / q2 of the actor (below)
        dirty[5 + row % 2][row] = bad
    logp_bad = dirty[2].copy()
    logp_bad[m // 2] = np.nan
    log_alpha = np.array([-0.7], np.float32)
    for tag, rows in (('clean', clean), ('dirty', dirty)):
        names = ('q1t', 'q2t', 'logp_next', 'rew', 'nonterminal', 'q1', 'q2')
        arrays = dict(zip(names, rows), log_alpha=log_alpha, logp_bad=logp_bad, g_la=np.full(1, S, np.float32), g_la_bad=np.full(1, S, np.float32),
                      partials=np.full(64, S, np.float64))
        for variant in ('v', 'd'):
            arrays.update({'c%s_%s' % (variant, k): np.full(m, S, np.float32) for k in CRITIC_OUT})
            arrays.update({'a%s_%s' % (variant, k): np.full(m, S, np.float32) for k in ACTOR_OUT})
        arrays['only_y'] = np.full(m, S, np.float32)
        d = Slack(arrays, slack)
        v = d.views
        p = lambda k: v[k].data_ptr()
        ins = {k: p(k) for k in names}
        inv_m = float(np.float32(1) / np.float32(m))
        for variant, kw in (('v', dict(alpha=0.2)), ('d', dict(log_alpha=p('log_alpha')))):
            call('eb_sac_critic', O.EbSacCriticArgs(m=m, gamma=0.99, reward_scale=2.5, inv_m=inv_m,
                                                   **dict(ins, **kw), **{k: p('c%s_%s' % (variant, k)) for k in CRITIC_OUT}))
            call('eb_sac_actor', O.EbSacActorArgs(m=m, q1=p('q1'), q2=p('q2'), logp=p('logp_next'), inv_m=inv_m, target_entropy=-2.0,
                                                 g_log_alpha=p('g_la') if variant == 'd' else None, partials=p('partials'), **kw,
                                                 **{k: p('a%s_%s' % (variant, k)) for k in ACTOR_OUT}))
        call('eb_sac_critic', O.EbSacCriticArgs(m=m, gamma=0.99, reward_scale=2.5, inv_m=inv_m, alpha=0.2, y=p('only_y'),
                                               **{k: ins[k] for k in names[:5]}))
        call('eb_sac_actor', O.EbSacActorArgs(m=m, q1=p('q1'), q2=p('q2'), logp=p('logp_bad'), inv_m=inv_m, target_entropy=-2.0, alpha=0.2,
                                             g_log_alpha=p('g_la_bad'), partials=p('partials')))
        have, untouched = d.host()
        assert untouched, tag
        for variant, kw in (('v', dict(alpha=0.2)), ('d', dict(log_alpha=log_alpha[0]))):
            want = O.critic_reference(*rows, gamma=0.99, reward_scale=2.5, inv_m=inv_m, **kw)
            for k in CRITIC_OUT:
                assert bits(have['c%s_%s' % (variant, k)], want[k]), (tag, variant, k)
            want = O.actor_reference(rows[5], rows[6], rows[2], inv_m=inv_m, target_entropy=-2.0, **kw)
            for k in ACTOR_OUT:
                assert bits(have['a%s_%s' % (variant, k)], want[k]), (tag, variant, k)
            if variant == 'd':
                assert bits(have['g_la'], want['g_log_alpha']) and np.isfinite(have['g_la']).all(), (tag, have['g_la'], want['g_log_alpha'])
            else:
                assert bits(have['only_y'], O.critic_reference(*rows, alpha=0.2, gamma=0.99, reward_scale=2.5, inv_m=inv_m)['y'])
        assert np.isnan(have['g_la_bad']).all()                              # a NaN row poisons g_log_alpha through S
        assert all(bits(have[k], arrays[k]) for k in names)
        if tag == 'clean':
            kept = have
        else:
            others = np.ones(m, bool)
            others[poisoned] = False
            for variant in ('v', 'd'):
                for k in ['c%s_%s' % (variant, k) for k in CRITIC_OUT] + ['a%s_%s' % (variant, k) for k in ACTOR_OUT if k != 'g_logp']:
                    assert bits(have[k][others], kept[k][others]), k      # the poisoned rows poison only themselves
                    assert not np.isfinite(have[k][poisoned]).all() or k.endswith(('g_q1', 'g_q2')) and k.startswith('a'), k


@pytest.mark.parametrize('slack', [4, 3])
@pytest.mark.parametrize('segments', [1, 2, 32])
def test_polyak_equals_the_restatement(segments, slack):
    counts = [(1, 255, 4097)[k % 3] for k in range(segments)]
    rng = np.random.default_rng(segments)
    arrays = {}
    for k, c in enumerate(counts):
        arrays['t%d' % k], arrays['o%d' % k] = rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    arrays['t0'][0], arrays['o0'][0] = (np.nan, 1.0) if segments == 2 else (0.5, np.inf)
    d = Slack(arrays, slack)
    v = d.views
    a = O.EbPolyakArgs(n_segments=segments, tau=0.005)
    for k, c in enumerate(counts):
        a.segments[k].target, a.segments[k].online, a.segments[k].count = v['t%d' % k].data_ptr(), v['o%d' % k].data_ptr(), c
    want = {k: x.copy() for k, x in arrays.items()}
    for rounds in range(2):
        call('eb_polyak', a)
        for k in range(segments):
            want['t%d' % k] = O.polyak_reference(want['t%d' % k], want['o%d' % k], 0.005)
    have, untouched = d.host()
    assert untouched and all(bits(have[k], want[k]) for k in arrays)
    assert not np.isfinite(have['t0'][0]) and np.isfinite(have['t0'][1:]).all()


def test_refusals_on_the_device_write_nothing():
    import torch
    x = torch.full((64,), S, device='cuda')
    p = x.data_ptr()
    api = O.offpolicy_api()
    for name, a in (('eb_q_pack', O.EbQPackArgs(m=4, obs_dim=3, act_dim=2, obs=p, act=p + 2, qin=p)),
                    ('eb_sac_critic', O.EbSacCriticArgs(m=4, q1t=p, q2t=p, logp_next=p, rew=p, nonterminal=p, alpha=float('nan'), y=p)),
                    ('eb_polyak', O.EbPolyakArgs(n_segments=33, tau=0.1)),
                    ('eb_q_action_grad', O.EbQActionGradArgs(m=4, obs_dim=3, act_dim=17, g_in1=p, g_a=p))):
        assert getattr(api.lib, name)(C.byref(a)) == -1 and api.lib.eb_offpolicy_last_error().startswith(name.encode() + b':'), name
    torch.cuda.synchronize()
    assert (x == S).all()
    with pytest.raises(ValueError, match='eb_replay_push'):
        api.check(api.push(C.byref(O.EbReplayPushArgs(capacity=4, n=5, obs_dim=1, act_dim=1))))


# ---- 3: streams and capture -------------------------------------------------------------------------------------------------------------------
def test_every_entry_on_a_side_stream_and_under_capture():
    """each of 'eb_replay_push', 'eb_replay_sample', 'eb_q_pack', 'eb_sac_critic', 'eb_sac_actor' (with and without g_log_alpha),
    'eb_q_action_grad' and 'eb_polyak' on the null stream, on a side stream and under capture: one kernel node (two with the temperature
    gradient), no other node kind, a chain; two replays advance what two eager calls advance."""
    import torch
    side = side_stream()
    m, D, A = 65, 41, 2
    buf = O.ReplayBuffer(130, D, A, 'cuda')
    rng = np.random.default_rng(4)
    st = {k: (gpu(a, np.uint8) if a.dtype == np.uint8 else gpu(a)) for k, a in T.step_arrays(m, D, A).items()}
    for k in T.RING:
        getattr(buf, k).copy_(gpu(T.ring_arrays(130, D, A, seed=1)[k]))
    buf.fill.fill_(100)
    new = lambda *s: gpu(rng.standard_normal(s))
    outs = dict(obs=buf.obs, act=buf.act, rew=buf.rew, next_obs=buf.next_obs, nonterminal=buf.nonterminal, fill=buf.fill,
                s_obs=new(m, D), s_qin=new(m, D + A), s_next=new(m, D), s_rew=new(m), s_nt=new(m), s_index=torch.zeros(m, dtype=torch.int32, device='cuda'),
                qin=new(m, D + A), y=new(m), loss1=new(m), loss2=new(m), g_q1=new(m), g_q2=new(m), aloss=new(m), ga_q1=new(m), ga_q2=new(m),
                g_logp=new(m), g_la=new(1), partials=torch.zeros(64, dtype=torch.float64, device='cuda'), g_a=new(m, A), target=new(300))
    rows = [gpu(x) for x in T.row_inputs(m)]
    online, log_alpha, g1, g2 = new(300), gpu(np.array([-0.3], np.float32)), new(m, D + A), new(m, D + A)
    first = {k: t.clone() for k, t in outs.items()}
    push = buf.push_args(m)
    push.start, push.fill_after = 120, 130
    push.prev_obs, push.action, push.reward, push.obs_after = (st[k].data_ptr() for k in ('prev_obs', 'action', 'reward', 'obs_after'))
    push.done_code, push.final_obs = st['done_code'].data_ptr(), st['final_obs'].data_ptr()
    sample = buf.sample_args(dict(obs=outs['s_obs'], qin=outs['s_qin'], next_obs=outs['s_next'], rew=outs['s_rew'], nonterminal=outs['s_nt'],
                                  index=outs['s_index']), seed=3, draw=1)
    critic = O._critic_args(*rows[:5], q1=rows[5], q2=rows[6], log_alpha=log_alpha, **{k: outs[k] for k in CRITIC_OUT})
    actor_kw = dict(log_alpha=log_alpha, loss=outs['aloss'], g_q1=outs['ga_q1'], g_q2=outs['ga_q2'], g_logp=outs['g_logp'])
    entries = (('eb_replay_push', push, T.RING + ('fill',), 1),
               ('eb_replay_sample', sample, ('s_obs', 's_qin', 's_next', 's_rew', 's_nt', 's_index'), 1),
               ('eb_q_pack', O._pack_args(outs['qin'], outs['s_obs'], outs['g_a']), ('qin',), 1),
               ('eb_sac_critic', critic, CRITIC_OUT, 1),
               ('eb_sac_actor', O._actor_args(rows[5], rows[6], rows[2], **actor_kw), ('aloss', 'ga_q1', 'ga_q2', 'g_logp'), 1),
               ('eb_sac_actor', O._actor_args(rows[5], rows[6], rows[2], target_entropy=-2.0, g_log_alpha=outs['g_la'], partials=outs['partials'],
                                              **actor_kw), ('aloss', 'ga_q1', 'ga_q2', 'g_logp', 'g_la', 'partials'), 2),
               ('eb_q_action_grad', O._action_grad_args(g1, g2, outs['g_a']), ('g_a',), 1),
               ('eb_polyak', O._polyak_args([(outs['target'], online)], 0.25), ('target',), 1))

    def start():
        for k, t in outs.items():
            t.copy_(first[k])
        torch.cuda.synchronize()

    def snap():
        torch.cuda.synchronize()
        return {k: host(t).copy() for k, t in outs.items()}

    for name, a, names, launches in entries:
        run = lambda s: call(name, a, s)
        start()
        before = snap()
        run(None)
        want = snap()
        assert not any(bits(want[k], before[k]) for k in names), name
        assert all(bits(want[k], before[k]) for k in outs if k not in names), name
        run(None)
        twice = snap()
        start()
        run(side.cuda_stream)
        assert all(bits(x, want[k]) for k, x in snap().items()), name
        start()
        cap = capture(side, run, name)
        try:
            assert all(bits(x, before[k]) for k, x in snap().items()), '%s ran under capture' % name
            nodes = dict(cap.node_types())
            print('%s:' % name, nodes)
            assert nodes == {'kernel': launches} and cap.is_chain(), name       # no memset, no memcpy
            cap.replay()
            assert all(bits(x, want[k]) for k, x in snap().items()), name
            cap.replay()
            assert all(bits(x, twice[k]) for k, x in snap().items()), name
        finally:
            cap.close()
    assert not bits(twice['target'], want['target'])


def test_a_captured_sample_sees_the_ring_grow_and_the_counter_move():
    """a captured eb_replay_sample replayed after a further push reads the new *fill, and replayed after eb_epoch_advance on its counter
    draws the next key's indices — as eager calls do"""
    import torch
    from env_build_amd import epoch
    side = side_stream()
    m, D, A, C_ = 33, 41, 2, 100
    buf = O.ReplayBuffer(C_, D, A, 'cuda')
    st = {k: (gpu(a, np.uint8) if a.dtype == np.uint8 else gpu(a)) for k, a in T.step_arrays(40, D, A).items()}
    buf.push(**st)
    counter = torch.zeros(1, dtype=torch.int64, device='cuda')
    batch = dict(obs=torch.zeros(m, D, device='cuda'), index=torch.zeros(m, dtype=torch.int32, device='cuda'))
    a = buf.sample_args(batch, seed=21, draw=0, counter=counter)
    cap = capture(side, lambda s: call('eb_replay_sample', a, s), 'eb_replay_sample')
    try:
        cap.replay()
        torch.cuda.synchronize()
        assert len(buf) == 40 and bits(host(batch['index']), O.sample_index_reference(m, 40, 21, 0).astype(np.int32))
        buf.push(**st)                                                        # the ring grows: *fill = 80
        cap.replay()
        torch.cuda.synchronize()
        grown = O.sample_index_reference(m, 80, 21, 0).astype(np.int32)
        assert bits(host(batch['index']), grown) and grown.max() >= 40
        with torch.cuda.stream(side):
            adv = epoch.EbEpochAdvanceArgs(counter=counter.data_ptr(), by=1, stream=side.cuda_stream)
            epoch.epoch_api().check(epoch.epoch_api().epoch_advance(C.byref(adv)))
        cap.replay()
        torch.cuda.synchronize()
        moved = O.sample_index_reference(m, 80, 21, 0, base=1).astype(np.int32)
        assert bits(host(batch['index']), moved) and not bits(moved, grown)
        assert bits(host(batch['obs']), O.sample_reference(buf.ring(), 80, m, 21, 0, base=1)['obs'])
        buf.sample_into(batch, seed=21, draw=1)                               # the eager twin: draw 1 without a counter
        torch.cuda.synchronize()
        assert bits(host(batch['index']), moved)
    finally:
        cap.close()


# ---- 4: the Collector ---------------------------------------------------------------------------------------------------------------------------
def make_env(limit=4):
    from env_build_amd.endtoend import CrossroadEnd2end
    env = CrossroadEnd2end('left', n_env=64, auto_reset=True, copy_outputs=False, max_episode_steps=limit)
    env.seed(0)
    env.reset()
    env.reset()
    return env


def make_policy():
    from tests import _epoch as E
    policy, _value = E.make_nets()
    policy.set_obs_scale(None)
    return policy


def test_collector_equals_a_loop_written_out():
    """two 64-env 'left' envs under one seed, policies of equal weights; one driven by offpolicy.Collector for 6 steps (the first two with
    the warm-up's actions), the other by the loop below — sample_from_logits / sample_actions, env.step, push_reference on the host.  The
    ring has 200 slots, so the 4th batch wraps and fill saturates."""
    import torch
    from env_build_amd.policy_sample import sample_actions, sample_from_logits
    B, seed, C_ = 64, 11, 200
    env_p, env_c = make_env(), make_env()
    D, A = env_p.obs_dim, env_p.action_number
    policy_p, policy_c = make_policy(), make_policy()
    buf = O.ReplayBuffer(C_, D, A, env_c.device)
    for k in T.RING:
        getattr(buf, k).fill_(S)
    col = O.Collector(env_c, policy_c, buf, 1.0, seed=seed)
    want = T.ring_arrays(C_, D, A, sentinel=True)
    finished = truncated = 0
    zero = torch.zeros((B, 2 * A), device='cuda')
    for t in range(6):
        prev = host(env_p.obs.t).copy()
        if t < 2:
            drawn = sample_from_logits(zero, 1.0, seed=seed, counter=t, want=())
        else:
            drawn = sample_actions(policy_p, gpu(prev), 1.0, seed=seed, counter=t, want=())
        obs, reward, _done, info = env_p.step(drawn['actions'])
        code, final = host(env_p.done_code), host(info['final_observation'].t)
        O.push_reference(want, (t * B) % C_, prev, host(drawn['actions'].t), host(reward.t), host(obs.t), code, final)
        slots = ((t * B) % C_ + np.arange(B)) % C_
        assert bits(want['next_obs'][slots[code != 0]], final[code != 0])          # a finished env's transition ends in its final observation
        assert bits(want['nonterminal'][slots], ((code == 0) | (code == 7)).astype(np.float32))
        finished, truncated = finished + int((code != 0).sum()), truncated + int((code == 7).sum())
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_stats()['allocation.all.allocated']
        col.random_steps(1) if t < 2 else col.step()
        assert t == 0 or torch.cuda.memory_stats()['allocation.all.allocated'] == allocated, t      # no allocation (the env's first step makes its own)
        torch.cuda.synchronize()
        have = buf.ring()
        for k in T.RING:
            assert bits(have[k], want[k]), (t, k)
        assert int(buf.fill.item()) == len(buf) == min((t + 1) * B, C_) and buf.cursor == ((t + 1) * B) % C_
    assert finished >= truncated > 0 and (want['obs'] != S).all()


# ---- 5: SAC ----------------------------------------------------------------------------------------------------------------------------------------
BATCH, GAMMA, TAU, LR = 65, 0.97, 0.05, 3e-3


def sac_nets():
    from env_build_amd.policy_grad import TrainableMLPNet
    from tests._ppo import make_net
    policy, p_layers, _ = make_net((41, 2, 64, 4, 'elu', 'linear'), False, TrainableMLPNet)
    p_layers = list(p_layers)
    p_layers[-1] = ((p_layers[-1][0] * np.float32(0.4)).astype(np.float32), p_layers[-1][1])
    policy.set_weights([a for pair in p_layers for a in pair])
    q1, _, _ = make_net((43, 2, 64, 1, 'elu', 'linear'), False, TrainableMLPNet)
    q2, layers, _ = make_net((43, 2, 64, 1, 'elu', 'linear'), False, TrainableMLPNet)
    q2.set_weights([(a * np.float32(0.9)).astype(np.float32) for pair in layers for a in pair])
    return policy, q1, q2


def sac_setup(capacity=300, filled=300):
    buf = O.ReplayBuffer(capacity, 41, 2, 'cuda')
    ring = T.ring_arrays(capacity, 41, 2, seed=8)
    ring['act'] = np.tanh(ring['act']).astype(np.float32)
    ring['nonterminal'] = (np.arange(capacity) % 5 != 0).astype(np.float32)
    for k in T.RING:
        getattr(buf, k).copy_(gpu(ring[k]))
    buf.fill.fill_(filled)
    buf.size = filled
    policy, q1, q2 = sac_nets()
    sac = O.SAC(policy, q1, q2, buf, BATCH, gamma=GAMMA, tau=TAU, lr=LR, log_alpha0=-0.5, reward_scale=2.0, action_range=1.0, seed=5)
    return sac, ring


def sac_state(sac):
    import torch
    torch.cuda.synchronize()
    out = {}
    for name, net, adam in (('pi', sac.policy, sac.adam_pi), ('q1', sac.q1, sac.adam_q1), ('q2', sac.q2, sac.adam_q2)):
        out[name], out[name + '_m'], out[name + '_v'] = host(net._flat).copy(), host(adam.m[0]).copy(), host(adam.v[0]).copy()
        out[name + '_adam'] = host(adam.state.buffer).copy()
    out.update(log_alpha=host(sac.log_alpha).copy(), alpha_m=host(sac.adam_alpha.m[0]).copy(), alpha_adam=host(sac.adam_alpha.state.buffer).copy(),
               t1=host(sac.target_flat[0]).copy(), t2=host(sac.target_flat[1]).copy(), counter=host(sac.counter).copy())
    return out


def written_out_step(sac, ring, f, state):
    """SAC.step()'s chain issued call by call through the module's and the package's existing functions on tensors of its own, every
    off-policy launch checked against its restatement; `state`: the networks, optimisers, targets and counter of a second SAC object, used
    as containers only (its step() is never called)"""
    import torch
    from env_build_amd import epoch
    from env_build_amd.policy_sample import sample_actions, sample_vjp
    n, D, A, api = sac.n, 41, 2, sac.api
    s = None
    new = lambda *shape: torch.zeros(shape, device='cuda')
    base = int(state.counter.item())
    mb = dict(obs=new(n, D), qin=new(n, D + A), next_obs=new(n, D), rew=new(n), nonterminal=new(n), noise_id=torch.zeros(n, dtype=torch.int32, device='cuda'))
    O.sample(state.buffer, mb, seed=state.seed, draw=0, counter=state.counter)
    want = O.sample_reference(ring, f, n, state.seed, 0, base=base)
    torch.cuda.synchronize()
    assert all(bits(host(mb[k]), want[k]) for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal')) and bits(host(mb['noise_id']), want['noise_id'].view(np.int32))
    sampled = {k: host(t).copy() for k, t in mb.items()}                       # (mb.qin's action columns are overwritten further down)
    nxt = sample_actions(state.policy, mb['next_obs'], 1.0, seed=state.seed, counter=0, row_ids=mb['noise_id'], want=('logp',))
    qin_next = O.q_pack(new(n, D + A), mb['next_obs'], nxt['actions'].t)
    assert bits(host(qin_next), O.q_pack_reference(np.zeros((n, D + A), np.float32), want['next_obs'], host(nxt['actions'].t)))
    fwd = lambda h, x: (lambda out: (api.mlp_forward(h, n, x.data_ptr(), out.data_ptr(), s), out)[1])(new(n))
    q1t, q2t = fwd(state.targets[0]._handle, qin_next), fwd(state.targets[1]._handle, qin_next)
    for q in (state.q1, state.q2, state.policy):
        q._sync()
    q1, q2 = fwd(state.q1._h, mb['qin']), fwd(state.q2._h, mb['qin'])
    c = {k: new(n) for k in CRITIC_OUT}
    O.sac_critic(q1t, q2t, nxt['logp'].t, mb['rew'], mb['nonterminal'], q1=q1, q2=q2, log_alpha=state.log_alpha, gamma=GAMMA, reward_scale=2.0, **c)
    wc = O.critic_reference(host(q1t), host(q2t), host(nxt['logp'].t), want['rew'], want['nonterminal'], host(q1), host(q2),
                            log_alpha=host(state.log_alpha)[0], gamma=GAMMA, reward_scale=2.0)
    assert all(bits(host(c[k]), wc[k]) for k in CRITIC_OUT)

    def backward(net, x, g_out, g_obs, g_params):
        ws, need = state._ws[net]
        api.mlp_backward(net._h, n, x.data_ptr(), g_out.data_ptr(), 0, 0.0, ws.data_ptr(), need, None, None if g_obs is None else g_obs.data_ptr(),
                         None if g_params is None else g_params.data_ptr(), s)
    for q, adam, g in ((state.q1, state.adam_q1, c['g_q1']), (state.q2, state.adam_q2, c['g_q2'])):
        backward(q, mb['qin'], g, None, adam.grads[0])
        adam.step(gather=False)
        q._sync()
    new_a = sample_actions(state.policy, mb['obs'], 1.0, seed=state.seed, counter=1, row_ids=mb['noise_id'], want=('logp', 'logits', 'eps'))
    O.q_pack(mb['qin'], None, new_a['actions'].t)
    assert bits(host(mb['qin']), np.concatenate([want['obs'], host(new_a['actions'].t)], axis=1))
    q1n, q2n = fwd(state.q1._h, mb['qin']), fwd(state.q2._h, mb['qin'])
    a = {k: new(n) for k in ACTOR_OUT}
    O.sac_actor(q1n, q2n, new_a['logp'].t, log_alpha=state.log_alpha, target_entropy=state.target_entropy, g_log_alpha=state.g_log_alpha,
                partials=state.partials, **a)
    wa = O.actor_reference(host(q1n), host(q2n), host(new_a['logp'].t), log_alpha=host(state.log_alpha)[0], target_entropy=state.target_entropy)
    assert all(bits(host(a[k]), wa[k]) for k in ACTOR_OUT) and bits(host(state.g_log_alpha), wa['g_log_alpha'])
    g_in1, g_in2 = new(n, D + A), new(n, D + A)
    backward(state.q1, mb['qin'], a['g_q1'], g_in1, None)
    backward(state.q2, mb['qin'], a['g_q2'], g_in2, None)
    g_a = O.q_action_grad(g_in1, g_in2, new(n, A))
    assert bits(host(g_a), O.action_grad_reference(host(g_in1), host(g_in2), A))
    g_logits = sample_vjp(new_a['logits'], new_a['eps'], 1.0, g_actions=g_a, g_logp=a['g_logp'])
    backward(state.policy, mb['obs'], g_logits.t, None, state.adam_pi.grads[0])
    state.adam_pi.step(gather=False)
    state.policy._sync()
    state.adam_alpha.issue()
    before = [host(t).copy() for t in state.target_flat]
    O.polyak(zip(state.target_flat, (state.q1._flat.detach(), state.q2._flat.detach())), TAU)
    for t, flat, b, q in zip(state.targets, state.target_flat, before, (state.q1, state.q2)):
        assert bits(host(flat), O.polyak_reference(b, host(q._flat), TAU))
        api.mlp_set_params_device(t._handle, flat.data_ptr(), s)
    adv = epoch.EbEpochAdvanceArgs(counter=state.counter.data_ptr(), by=1, stream=s)
    epoch.epoch_api().check(epoch.epoch_api().epoch_advance(C.byref(adv)))
    return dict(grads=[host(x.grads[0]).copy() for x in (state.adam_pi, state.adam_q1, state.adam_q2)], g_log_alpha=host(state.g_log_alpha).copy(),
                mb=sampled, eps_new=host(new_a['eps'].t).copy(), a_next=host(nxt['actions'].t).copy())


def test_sac_step_equals_the_chain_written_out_and_its_graph():
    """two SAC.step()s against the chain issued call by call (every parameter tensor, Adam state, log_alpha, target tensor and the draw
    counter bit-equal), then capture() and two replays against two eager steps; the graph holds SAC.KERNELS kernel nodes and nothing
    else; no allocation."""
    import torch
    sac, ring = sac_setup()
    twin, _ = sac_setup()
    start = sac_state(sac)
    assert all(bits(x, sac_state(twin)[k]) for k, x in start.items())
    sac.step()                                                                 # (the first call binds what is bound on first use)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    sac.step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    for k in range(2):
        written_out_step(sac, ring, 300, twin)
    eager = sac_state(sac)
    for k, x in sac_state(twin).items():
        assert bits(x, eager[k]), k
    assert eager['counter'].tolist() == [2] and not bits(eager['pi'], start['pi']) and not bits(eager['t1'], start['t1'])
    assert not bits(eager['log_alpha'], start['log_alpha'])
    log = sac.log()
    assert sorted(log) == ['actor_loss', 'alpha', 'critic1_loss', 'critic2_loss', 'logp', 'y'] and all(np.isfinite(x) for x in log.values())
    assert abs(log['alpha'] - float(np.exp(eager['log_alpha'][0]))) < 1e-5
    # the graph
    fresh, _ = sac_setup()
    graph = fresh.capture(keep_graph=True)
    cap = Captured(graph, torch.cuda.current_stream(), 'SAC.step')
    nodes = dict(cap.node_types())
    print('SAC.step graph:', nodes)
    assert nodes == {'kernel': O.SAC.KERNELS} and cap.is_chain()
    assert all(bits(x, start[k]) for k, x in sac_state(fresh).items())        # nothing ran during the capture
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    fresh.replay(graph)
    fresh.replay(graph)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    for k, x in sac_state(fresh).items():
        assert bits(x, eager[k]), k


def test_wiring_against_an_independent_differentiation():
    """the same sampled batch and the same noise through a torch twin of the three losses under autograd, in float64 and in float32:
    per tensor |g - g64|_inf <= 2 |g32 - g64|_inf — the bar computed from the run itself, the factor 2 for the differing summation orders.
    Worst ratio seen: 0.72 (the policy's gradient)."""
    import torch
    sac, ring = sac_setup()
    twin, _ = sac_setup()
    w0 = {name: [torch.from_numpy(a) for a in net.get_weights()] for name, net in (('pi', sac.policy), ('q1', sac.q1), ('q2', sac.q2))}
    out = written_out_step(sac, ring, 300, twin)                               # (sac: the shapes only)
    mb, log_alpha0 = out['mb'], -0.5
    t1, t2 = w0['q1'], w0['q2']                                                # the targets start as copies of the critics

    def mlp(ws, x):
        for k in range(0, len(ws) - 2, 2):
            x = torch.nn.functional.elu(x @ ws[k] + ws[k + 1])
        return x @ ws[-2] + ws[-1]

    def squash(logits, eps):
        mean, ls = logits[:, :2], logits[:, 2:]
        u = mean + torch.exp(ls) * eps
        a = torch.tanh(u)
        logp = (-0.5 * eps * eps - ls - 0.5 * np.log(2 * np.pi)).sum(1) - (2.0 * (np.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(1)
        return a, logp

    # the twin proper: the noise of both samples is the library's own (eps of the new action is an output; the next action's noise is
    # policy_noise_reference's under the same row ids)
    from env_build_amd.policy_sample import policy_noise_reference
    ids = mb['noise_id'].view(np.uint32)
    eps_next, eps_new = policy_noise_reference(ids, 2, 5, 0), out['eps_new']
    assert bits(policy_noise_reference(ids, 2, 5, 1), eps_new)
    results = {}
    for dtype in (torch.float64, torch.float32):
        c = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
        P = {k: [c(a.numpy()).clone().requires_grad_(True) for a in ws] for k, ws in w0.items()}
        la = c(np.float32(log_alpha0)).clone().requires_grad_(True)
        obs, qin, nxt, rew, nt = (c(mb[k]) for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal'))
        with torch.no_grad():
            a_next, logp_next = squash(mlp(P['pi'], nxt), c(eps_next))
            x = torch.cat([nxt, a_next], 1)
            qm = torch.minimum(mlp([c(a.numpy()) for a in t1], x), mlp([c(a.numpy()) for a in t2], x))[:, 0]
            y = 2.0 * rew + GAMMA * nt * (qm - torch.exp(la) * logp_next)
        critic = sum((0.5 * (mlp(P[k], qin)[:, 0] - y) ** 2).mean() for k in ('q1', 'q2'))
        gq = torch.autograd.grad(critic, P['q1'] + P['q2'])
        # the critics after their Adam step are the library's own: the actor loss is differentiated at THOSE weights
        Q = {k: [c(a) for a in net.get_weights()] for k, net in (('q1', twin.q1), ('q2', twin.q2))}
        a_new, logp = squash(mlp(P['pi'], obs), c(eps_new))
        x = torch.cat([obs, a_new], 1)
        actor = (torch.exp(la).detach() * logp - torch.minimum(mlp(Q['q1'], x), mlp(Q['q2'], x))[:, 0]).mean()
        gp = torch.autograd.grad(actor, P['pi'])
        temp = -(la * (logp.detach() + (-2.0)).mean())
        gla = torch.autograd.grad(temp, la)
        flat = lambda gs: torch.cat([g.reshape(-1) for g in gs]).double().numpy()
        results[dtype] = dict(q1=flat(gq[:len(P['q1'])]), q2=flat(gq[len(P['q1']):]), pi=flat(gp), log_alpha=flat(gla))
    have = dict(pi=out['grads'][0], q1=out['grads'][1], q2=out['grads'][2], log_alpha=out['g_log_alpha'])
    worst = 0.0
    for k in ('q1', 'q2', 'pi', 'log_alpha'):
        g64, g32 = results[torch.float64][k], results[torch.float32][k]
        err, bar = np.abs(have[k].astype(np.float64) - g64).max(), 2.0 * np.abs(g32 - g64).max()
        print('wiring %s: |g - g64| = %.3e, |g32 - g64| = %.3e, ratio to the bar %.3f (|g64| max %.3e)' % (k, err, bar / 2, err / bar, np.abs(g64).max()))
        assert np.abs(g64).max() > 1e-4, k
        worst = max(worst, err / bar)
        assert err <= bar, (k, err, bar)
    print('wiring: worst ratio %.3f' % worst)


# ---- 6: the example ------------------------------------------------------------------------------------------------------------------------------
def test_sac_env_loop_example_runs():
    spec = importlib.util.spec_from_file_location('sac_env_loop', os.path.join(ROOT, 'examples', 'sac_env_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    logs = mod.main(['--iterations', '3', '--n-env', '64', '--warmup', '2', '--batch', '64', '--capacity', '1000', '--hidden', '64'])
    assert len(logs) == 3
    for log in logs:
        assert all(np.isfinite(v) for v in log.values()), log
