"""GPU (-m gpu): the prioritised-replay family on the MI355X, array_equal to the NumPy restatements of env_build_amd.per — the tree's
invariant after every write on both routes, the draw on the keyed route and through u_in with every prefix boundary and the fallback, the
weights and new priorities, every entry on a side stream and under capture with the launch counts read from the graph, and `per.SAC`:
the leaves, the tree and the weighted cotangents of one step, a captured replay against an eager step, two replays drawing two batches.
Every array of the entry tests is a view into the middle of a larger allocation whose slack must stay as made."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from env_build_amd import offpolicy as O
from env_build_amd import per as P
from tests import _per as T
from tests._capture import Captured, capture, side_stream
from tests._helpers import ROOT
from tests._per import bits
from tests._ppo import gpu

pytestmark = pytest.mark.gpu

R, X = P.EB_PER_ROUTE_RANGE, P.EB_PER_ROUTE_INDEXED


def host(t):
    return t.detach().cpu().numpy()


def call(name, a, stream=None):
    api = P.per_api()
    a.stream = stream
    api.check(getattr(api.lib, name)(C.byref(a)))


class Structure(P.PrioritizedReplayBuffer):
    """the structure of a PrioritizedReplayBuffer without its ring, every array a view into the middle of a larger one: three sentinel
    elements either side of prio, stamp and max_prio (an odd float offset), one either side of the tree (doubles stay 8-byte aligned)"""

    def __init__(self, C_):
        import torch
        from env_build_amd.dynamics_and_models import _resolve_device
        self.capacity, self.device, self.api = C_, _resolve_device('cuda'), P.per_api()
        self.big = dict(prio=torch.full((C_ + 6,), T.SENTINEL, device='cuda'), stamp=torch.full((C_ + 6,), -77, dtype=torch.int32, device='cuda'),
                        max_prio=torch.full((7,), T.SENTINEL, device='cuda'),
                        tree=torch.full((P.tree_doubles(C_) + 2,), T.SENTINEL, dtype=torch.float64, device='cuda'))
        self.prio, self.stamp, self.max_prio = self.big['prio'][3:-3], self.big['stamp'][3:-3], self.big['max_prio'][3:-3]
        self.tree = self.big['tree'][1:-1]
        assert self.tree.data_ptr() % 8 == 0 and self.prio.data_ptr() % 8 == 4

    def load(self, prio, max_prio=1.0, tree=None):
        """a state put there directly: the leaves, the tree built from them by tree_reference (or the one given), stamps at rest"""
        import torch
        self.prio.copy_(gpu(np.array(prio)))                               # (a copy: the shared cases are read-only arrays)
        self.tree.copy_(gpu(P.tree_reference(prio) if tree is None else tree, np.float64))
        self.max_prio.fill_(float(max_prio))
        self.stamp.fill_(-1)
        torch.cuda.synchronize()

    def check(self, prio, max_prio, what):
        """the device state against the restatement: leaves, the tree rebuilt from them, max_prio, stamps at rest, the slack"""
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(host(self.prio), prio), what
        assert np.array_equal(host(self.tree), P.tree_reference(prio)), what
        assert host(self.max_prio).tolist() == [np.float32(max_prio)], what
        assert (host(self.stamp) == -1).all(), what
        for k, n in (('prio', 3), ('stamp', 3), ('max_prio', 3), ('tree', 1)):
            big = host(self.big[k])
            fill = -77 if k == 'stamp' else T.SENTINEL
            assert (big[:n] == fill).all() and (big[-n:] == fill).all(), (what, k)


# ---- 1: the invariant after every write ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_the_tree_meets_the_invariant_after_every_write(C_):
    """reset from garbage; the range route without a wrap, across it and over the whole ring; the indexed route at m in {1, 64, 257} with
    the rows that must be skipped or clamped, all rows naming one leaf, and every leaf named twice — the leaves, the rebuilt tree,
    max_prio and the stamps compared after each call"""
    s = Structure(C_)
    s.prio.fill_(3.0), s.tree.fill_(-5.0), s.max_prio.fill_(9.0), s.stamp.fill_(12)
    call('eb_per_reset', s.reset_args())
    prio, mx = np.zeros(C_, np.float32), np.float32(1)
    s.check(prio, mx, 'reset')
    steps = [('range', 0, 1), ('indexed', 64, 'random'), ('range', C_ // 2, C_ - C_ // 2), ('indexed', 1, 'random'), ('range', C_ - 1, min(C_, 3)),
             ('indexed', 257, 'random'), ('indexed', 257, 'one'), ('range', C_ // 3, C_), ('indexed', 2 * C_, 'twice'), ('range', C_ - 1, 1)]
    raised = False
    for k, (route, a, b) in enumerate(steps):
        if route == 'range':
            call('eb_per_set', s.set_args(R, b, start=a))
            prio, mx = P.set_reference(prio, mx, start=a, n=b)
        else:
            idx, val = T.write_back_rows(C_, a, b, seed=k)
            call('eb_per_set', s.set_args(X, len(idx), index=gpu(idx, np.int32), value=gpu(val)))
            prio, new_mx = P.set_reference(prio, mx, index=idx, value=val)
            raised, mx = raised or new_mx > mx, new_mx
        s.check(prio, mx, (C_, k, route, a, b))
    assert raised and (prio > 0).all() and mx > 1


# ---- 2: the draw -------------------------------------------------------------------------------------------------------------------------------
def draw(s, m, **kw):
    import torch
    out = dict(index=torch.full((m,), -77, dtype=torch.int32, device='cuda'), prio=torch.full((m,), T.SENTINEL, device='cuda'),
               noise_id=torch.full((m,), -77, dtype=torch.int32, device='cuda'), min_partials=torch.full((64,), T.SENTINEL, device='cuda'))
    call('eb_per_sample', s.draw_args(out['index'], out['prio'], out['noise_id'], out['min_partials'], **kw))
    torch.cuda.synchronize()
    return dict(index=host(out['index']), prio=host(out['prio']), noise_id=host(out['noise_id']).view(np.uint32), min_partials=host(out['min_partials']))


def same(have, want, what):
    for k in ('index', 'prio', 'noise_id', 'min_partials'):
        assert bits(have[k], want[k]), (what, k)


@pytest.mark.parametrize('m', [1, 63, 64, 65, 4096])
def test_sample_equals_the_restatement(m):
    """every capacity of the list, the last quarter of the ring never written (fill < C) and zero leaves interleaved in the rest; the keyed
    route without and with a device counter, and u_in"""
    import torch
    counter = torch.full((1,), 5, dtype=torch.int64, device='cuda')
    rng = np.random.default_rng(m)
    for C_ in T.CAPACITIES:
        prio = T.leaves(C_).copy()
        if C_ >= 4:
            prio[C_ - C_ // 4:] = 0
        s = Structure(C_)
        s.load(prio)
        same(draw(s, m, seed=9, draw=3), P.sample_reference(prio, m, 9, 3), (C_, 'keyed'))
        with_counter = draw(s, m, seed=9, draw=1, counter=counter)
        same(with_counter, P.sample_reference(prio, m, 9, 1, base=5), (C_, 'counter'))
        u_in = rng.uniform(size=m)
        u_in[0], u_in[-1] = 0.0, np.nextafter(1.0, 0.0)
        through = draw(s, m, seed=9, draw=1, counter=counter, u_in=gpu(u_in, np.float64))
        same(through, P.sample_reference(prio, m, 9, 1, base=5, u_in=u_in), (C_, 'u_in'))
        assert (prio[through['index']] > 0).all() and through['index'].max() < C_ - C_ // 4 or C_ < 4
        s.check(prio, 1.0, (C_, 'the draw writes nothing'))
    assert not bits(with_counter['index'], through['index'])


@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_boundaries_the_fallback_a_lone_leaf_and_an_empty_ring(C_):
    """the host file's cases on the device: one double step below and exactly at every prefix boundary; a stored sum beyond what the
    leaves reach (the last positive leaf); one positive leaf in the last slot; total == 0 (-1, NaN, +inf)"""
    s = Structure(C_)
    prio, u_in, want = T.boundary_case(C_)
    s.load(prio)
    have = draw(s, len(u_in), u_in=gpu(np.array(u_in), np.float64))
    assert np.array_equal(have['index'], want)
    same(have, P.sample_reference(prio, len(u_in), u_in=u_in), 'boundaries')
    prio, tree, u_in, last = T.fallback_case(C_)
    s.load(prio, tree=tree)
    have = draw(s, 1, u_in=gpu(u_in, np.float64))
    assert have['index'].tolist() == [last] and have['prio'][0] == prio[last] > 0
    lone = np.zeros(C_, np.float32)
    lone[C_ - 1] = 3.5
    s.load(lone)
    have = draw(s, 257, seed=9)
    assert (have['index'] == C_ - 1).all()
    same(have, P.sample_reference(lone, 257, seed=9), 'lone')
    s.load(np.zeros(C_, np.float32))
    have = draw(s, 65, seed=1)
    assert (have['index'] == -1).all() and (have['prio'].view(np.uint32) == 0x7FC00000).all() and np.isinf(have['min_partials']).all()
    same(have, P.sample_reference(np.zeros(C_, np.float32), 65, seed=1), 'empty')


def test_an_empty_draw_gathers_rows_of_nans():
    """index_out = -1 is what eb_replay_sample turns into a row of NaNs: a PrioritizedReplayBuffer before its first push"""
    import torch
    buf = P.PrioritizedReplayBuffer(40, 3, 2, 'cuda')
    batch = dict(index=torch.zeros(5, dtype=torch.int32, device='cuda'), obs=torch.zeros(5, 3, device='cuda'), rew=torch.zeros(5, device='cuda'))
    buf.sample_into(batch, seed=1)
    torch.cuda.synchronize()
    assert (host(batch['index']) == -1).all() and np.isnan(host(batch['obs'])).all() and np.isnan(host(batch['rew'])).all()


# ---- 3: the weight and the new priority ---------------------------------------------------------------------------------------------------------
WEIGH_OUT = ('g_q1', 'g_q2', 'loss1', 'loss2')


@pytest.mark.parametrize('alpha', [1.0, 0.6])
@pytest.mark.parametrize('m', [1, 65, 257])
def test_weigh_equals_the_restatement(m, alpha):
    """beta by value and from the device counter (annealing, and clamped at 1), both critics and q2 NULL, rows never drawn (-1) and NaN TD
    errors; the cotangents and losses are scaled in place"""
    import torch
    rows = T.weigh_rows(m, seed=3, nan=True, undrawn=True)
    dev = {k: gpu(v, v.dtype.type) for k, v in rows.items()}
    first = {k: dev[k].clone() for k in WEIGH_OUT}
    counter = torch.zeros(1, dtype=torch.int64, device='cuda')
    for name, kw, ref in (('value', dict(beta=0.4), dict(beta=0.4)),
                          ('counter 7', dict(beta=0.4, beta_step=0.01, counter=counter), dict(beta=0.4, beta_step=0.01, counter=7)),
                          ('counter 700', dict(beta=0.4, beta_step=0.01, counter=counter), dict(beta=0.4, beta_step=0.01, counter=700)),
                          ('one critic', dict(beta=1.0, q2=None), dict(beta=1.0, q2=None))):
        counter.fill_(ref.get('counter', 0))
        for k in WEIGH_OUT:
            dev[k].copy_(first[k])
        w, new = torch.full((m,), T.SENTINEL, device='cuda'), torch.full((m,), T.SENTINEL, device='cuda')
        tensors = dict(dev, **{k: v for k, v in kw.items() if k == 'q2'})
        args = {k: v for k, v in kw.items() if k != 'q2'}
        call('eb_per_weigh', P._weigh_args(tensors['index'], tensors['prio'], tensors['min_partials'], q1=tensors['q1'], q2=tensors['q2'], y=tensors['y'],
                                           alpha=alpha, eps=1e-3, w_out=w, prio_new=new, **{k: tensors[k] for k in WEIGH_OUT}, **args))
        torch.cuda.synchronize()
        given = dict(rows, **{k: v for k, v in ref.items() if k == 'q2'})
        want = P.weigh_reference(alpha=alpha, eps=1e-3, **given, **{k: v for k, v in ref.items() if k != 'q2'})
        assert bits(host(w), want['w']) and bits(host(new), want['prio_new']), name
        for k in WEIGH_OUT:
            assert bits(host(dev[k]), want[k]), (name, k)
        drawn = rows['index'] >= 0
        assert (host(w)[~drawn] == 0).all() and np.isnan(host(new)[~drawn]).all() and (host(w) <= 1).all()
        assert m < 12 or np.isnan(host(new)[::11]).all()
    assert P.beta_reference(0.4, 0.01, 700) == 1


# ---- 4: streams, capture and the launch counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', [1025, 32769, 2 ** 20 + 1])
def test_every_entry_on_a_side_stream_and_under_capture(C_):
    """each of 'eb_per_reset', 'eb_per_set' (both routes), 'eb_per_sample' and 'eb_per_weigh' on the null stream, on a side stream and
    under capture: kernel nodes only, a chain, as many as eb_per_set_launches says (0, 1 and 2 big levels); two replays leave what two
    eager calls leave"""
    import torch
    side = side_stream()
    m = 65
    s = Structure(C_)
    prio0 = T.leaves(C_)
    tree0 = P.tree_reference(prio0)
    idx, val = T.write_back_rows(C_, m, 'random')
    rows = T.weigh_rows(m, seed=1)
    dev = {k: gpu(v, v.dtype.type) for k, v in rows.items()}
    outs = dict(prio=s.prio, tree=s.tree, max_prio=s.max_prio, stamp=s.stamp, index=torch.zeros(m, dtype=torch.int32, device='cuda'),
                drawn=torch.zeros(m, device='cuda'), partials=torch.zeros(64, device='cuda'), g_q1=dev['g_q1'], loss2=dev['loss2'],
                w=torch.zeros(m, device='cuda'), new=torch.zeros(m, device='cuda'))
    first = {k: t.clone() for k, t in outs.items()}
    first['prio'], first['tree'] = gpu(prio0), gpu(tree0, np.float64)
    first['max_prio'], first['stamp'] = torch.ones(1, device='cuda'), torch.full((C_,), -1, dtype=torch.int32, device='cuda')
    lib = P.per_api().lib
    structure = ('prio', 'tree', 'max_prio')
    entries = (('eb_per_reset', s.reset_args(), ('prio', 'tree'), 1),
               ('eb_per_set', s.set_args(R, min(C_, 300), start=C_ - 40), ('prio', 'tree'), lib.eb_per_set_launches(C_, R)),
               ('eb_per_set', s.set_args(X, m, index=gpu(idx, np.int32), value=gpu(val)), structure, lib.eb_per_set_launches(C_, X)),
               ('eb_per_sample', s.draw_args(outs['index'], outs['drawn'], None, outs['partials'], seed=3, draw=1), ('index', 'drawn', 'partials'), 1),
               ('eb_per_weigh', P._weigh_args(dev['index'], dev['prio'], dev['min_partials'], q1=dev['q1'], q2=dev['q2'], y=dev['y'], beta=0.5,
                                              g_q1=outs['g_q1'], loss2=outs['loss2'], w_out=outs['w'], prio_new=outs['new']),
                ('g_q1', 'loss2', 'w', 'new'), 1))
    big = P.tree_levels(C_)[2] - 1
    assert [e[3] for e in entries] == [1, big + 2, big + 3, 1, 1] and big == {1025: 0, 32769: 1, 2 ** 20 + 1: 2}[C_]

    def start():
        for k, t in outs.items():
            t.copy_(first[k])
        torch.cuda.synchronize()

    def snap():
        torch.cuda.synchronize()
        return {k: host(t).copy() for k, t in outs.items()}

    for name, a, names, launches in entries:
        run = lambda stream: call(name, a, stream)
        start()
        before = snap()
        run(None)
        want = snap()
        assert not any(bits(want[k], before[k]) for k in names), (name, a.route if name == 'eb_per_set' else '')
        assert all(bits(want[k], before[k]) for k in outs if k not in names), name
        if name != 'eb_per_reset':
            assert np.array_equal(want['tree'], P.tree_reference(want['prio'])) and (want['stamp'] == -1).all(), name
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
            print('%s at C = %d:' % (name, C_), nodes)
            assert nodes == {'kernel': launches} and cap.is_chain(), name         # no memset, no memcpy
            cap.replay()
            assert all(bits(x, want[k]) for k, x in snap().items()), name
            cap.replay()
            assert all(bits(x, twice[k]) for k, x in snap().items()), name
        finally:
            cap.close()
    assert not bits(twice['g_q1'], want['g_q1'])                                  # the weights are applied in place: twice is not once


# ---- 5: the buffer and the collector ---------------------------------------------------------------------------------------------------------------
def test_buffer_push_sample_and_update_keep_the_invariant():
    """PrioritizedReplayBuffer: pushes across the wrap give the new slots max_prio; sample_into draws, gathers those rows and never a
    slot that was not written; update_priorities is the indexed route"""
    import torch
    from tests import _offpolicy as TO
    C_, D, A, n, m = 100, 5, 2, 40, 33
    buf = P.PrioritizedReplayBuffer(C_, D, A, 'cuda')
    st = {k: (gpu(a, np.uint8) if a.dtype == np.uint8 else gpu(a)) for k, a in TO.step_arrays(n, D, A).items()}
    prio, mx = np.zeros(C_, np.float32), np.float32(1)
    batch = dict(index=torch.zeros(m, dtype=torch.int32, device='cuda'), prio=torch.zeros(m, device='cuda'), obs=torch.zeros(m, D, device='cuda'),
                 rew=torch.zeros(m, device='cuda'), min_partials=torch.zeros(64, device='cuda'))
    for k in range(3):                                                             # 120 rows into 100 slots: the third push wraps
        start = buf.cursor
        buf.push(**st)
        prio, mx = P.set_reference(prio, mx, start=start, n=n)
        buf.sample_into(batch, seed=4, draw=k)
        want = P.sample_reference(prio, m, seed=4, draw=k)
        torch.cuda.synchronize()
        have = buf.structure()
        assert np.array_equal(have['prio'], prio) and np.array_equal(have['tree'], P.tree_reference(prio)) and have['max_prio'][0] == mx
        idx = host(batch['index'])
        assert np.array_equal(idx, want['index']) and bits(host(batch['prio']), want['prio']) and bits(host(batch['min_partials']), want['min_partials'])
        assert (idx < len(buf)).all() and bits(host(batch['obs']), buf.ring()['obs'][idx]) and bits(host(batch['rew']), buf.ring()['rew'][idx])
        value = gpu(np.linspace(0.5, 40.0, m) * (k + 1))
        buf.update_priorities(batch['index'], value)
        prio, mx = P.set_reference(prio, mx, index=idx, value=host(value))
    torch.cuda.synchronize()
    have = buf.structure()
    assert np.array_equal(have['prio'], prio) and np.array_equal(have['tree'], P.tree_reference(prio)) and have['max_prio'][0] == mx > 1
    assert (have['stamp'] == -1).all() and len(buf) == C_ and buf.cursor == 20


def test_collector_adds_the_range_route_to_the_parents_launches():
    """per.Collector against offpolicy.Collector under one seed: the same ring, and after every step the leaves of the slots written so
    far at max_prio (1: nothing raised it) and the tree rebuilt from them"""
    import torch
    from tests.test_gpu_offpolicy import make_env, make_policy
    C_ = 200
    env_a, env_b = make_env(), make_env()
    D, A = env_a.obs_dim, env_a.action_number
    plain, pri = O.ReplayBuffer(C_, D, A, env_a.device), P.PrioritizedReplayBuffer(C_, D, A, env_b.device)
    col_a, col_b = O.Collector(env_a, make_policy(), plain, 1.0, seed=11), P.Collector(env_b, make_policy(), pri, 1.0, seed=11)
    prio = np.zeros(C_, np.float32)
    for t in range(4):                                                             # 256 rows into 200 slots
        start = pri.cursor
        for col in (col_a, col_b):
            col.random_steps(1) if t < 2 else col.step()
        prio, _ = P.set_reference(prio, 1.0, start=start, n=64)
        torch.cuda.synchronize()
        a, b = plain.ring(), pri.ring()
        assert all(bits(a[k], b[k]) for k in a) and pri.cursor == plain.cursor and len(pri) == len(plain)
        have = pri.structure()
        assert np.array_equal(have['prio'], prio) and np.array_equal(have['tree'], P.tree_reference(prio)), t
    assert (prio == 1).all()
    with pytest.raises(TypeError):
        P.Collector(env_a, make_policy(), plain, 1.0)


# ---- 6: per.SAC ------------------------------------------------------------------------------------------------------------------------------------
PER_KW = dict(alpha=0.6, beta0=0.4, beta_step=0.25, eps=1e-3)


def per_setup(capacity=300, filled=300):
    """tests/test_gpu_offpolicy.py's SAC case — its ring, its networks, batch 65 — on a PrioritizedReplayBuffer whose priorities are put
    there through the library: max_prio over the filled slots, then a write-back of spread values over two thirds of them"""
    import torch
    from tests import _offpolicy as TO
    from tests.test_gpu_offpolicy import BATCH, GAMMA, LR, TAU, sac_nets
    buf = P.PrioritizedReplayBuffer(capacity, 41, 2, 'cuda')
    ring = TO.ring_arrays(capacity, 41, 2, seed=8)
    ring['act'] = np.tanh(ring['act']).astype(np.float32)
    ring['nonterminal'] = (np.arange(capacity) % 5 != 0).astype(np.float32)
    for k in TO.RING:
        getattr(buf, k).copy_(gpu(ring[k]))
    buf.fill.fill_(filled)
    buf.size = filled
    P.set_range(buf, 0, filled)
    rng = np.random.default_rng(31)
    idx = rng.permutation(filled)[:2 * filled // 3].astype(np.int32)
    val = np.exp(rng.uniform(np.log(0.05), np.log(20.0), len(idx))).astype(np.float32)
    buf.update_priorities(gpu(idx, np.int32), gpu(val))
    policy, q1, q2 = sac_nets()
    sac = P.SAC(policy, q1, q2, buf, BATCH, gamma=GAMMA, tau=TAU, lr=LR, log_alpha0=-0.5, reward_scale=2.0, action_range=1.0, seed=5, **PER_KW)
    torch.cuda.synchronize()
    return sac, ring


def per_state(sac):
    from tests.test_gpu_offpolicy import sac_state
    out = sac_state(sac)
    out.update(sac.buffer.structure())
    out.update(index=host(sac.mb.index).copy(), w=host(sac.rows.w).copy(), g_q1=host(sac.rows.g_q1).copy(), loss1=host(sac.rows.loss1).copy())
    return out


def test_per_sac_wiring_and_graph():
    """one step(): the batch is sample_reference's draw from the leaves before it, gathered; w and prio_new are weigh_reference of the step's
    own q1, q2, y at beta0 (counter 0); the leaves are set_reference's, the tree the rebuild; the cotangents that reach the critics'
    backward passes are exactly w times the uniform path's (critic_reference on the same rows).  Then the graph: sac.KERNELS kernel nodes
    = 42 + 2 + eb_per_set_launches(C, indexed), a chain; one replay equals one eager step() from the same state bit for bit, a second
    replay draws another batch at the next beta."""
    import torch
    from tests.test_gpu_offpolicy import BATCH, GAMMA
    sac, ring = per_setup()
    n, buf, r, mb = BATCH, sac.buffer, sac.rows, sac.mb
    start = per_state(sac)
    assert (start['prio'] > 0).all() and len(np.unique(start['prio'])) > 100 and start['max_prio'][0] > 1
    assert np.array_equal(start['tree'], P.tree_reference(start['prio']))
    sac.step()
    torch.cuda.synchronize()
    eager = per_state(sac)
    drawn = P.sample_reference(start['prio'], n, seed=5, draw=0, base=0)
    assert np.array_equal(eager['index'], drawn['index']) and bits(host(mb.prio), drawn['prio']) and bits(host(sac.min_partials), drawn['min_partials'])
    assert bits(host(mb.noise_id).view(np.uint32), drawn['noise_id']) and len(np.unique(drawn['index'])) > 30
    rows = O.sample_reference(ring, 300, n, indices=drawn['index'])
    assert bits(host(mb.obs), rows['obs']) and bits(host(mb.rew), rows['rew']) and bits(host(mb.next_obs), rows['next_obs'])
    q1, q2, y = host(r.q1), host(r.q2), host(r.y)
    uniform = O.critic_reference(host(r.q1t), host(r.q2t), host(r.logp_next), rows['rew'], rows['nonterminal'], q1, q2, log_alpha=start['log_alpha'][0],
                                 gamma=GAMMA, reward_scale=2.0)
    assert bits(y, uniform['y'])
    want = P.weigh_reference(drawn['index'], drawn['prio'], drawn['min_partials'], q1=q1, q2=q2, y=y, beta=0.4, beta_step=0.25, counter=0, alpha=0.6,
                             eps=1e-3, **{k: uniform[k] for k in WEIGH_OUT})
    assert bits(eager['w'], want['w']) and bits(host(r.prio_new), want['prio_new']) and want['w'].max() == 1 and want['w'].min() < 0.9
    for k in WEIGH_OUT:
        assert bits(host(getattr(r, k)), want[k]) and bits(want[k], uniform[k] * want['w']), k           # exactly w x the uniform path's
    prio, mx = P.set_reference(start['prio'], start['max_prio'][0], index=drawn['index'], value=want['prio_new'])
    assert np.array_equal(eager['prio'], prio) and eager['max_prio'][0] == mx and np.array_equal(eager['tree'], P.tree_reference(prio))
    assert np.array_equal(eager['prio'][drawn['index']], prio[drawn['index']]) and (eager['stamp'] == -1).all()
    assert not bits(eager['prio'], start['prio']) and eager['counter'].tolist() == [1]
    log = sac.log()
    assert sorted(log) == ['actor_loss', 'alpha', 'beta', 'critic1_loss', 'critic2_loss', 'logp', 'weight', 'y']
    assert abs(log['weight'] - float(want['w'].astype(np.float64).mean())) < 1e-7 and log['beta'] == float(np.float32(0.4))
    # the graph
    fresh, _ = per_setup()
    assert all(bits(x, start[k]) for k, x in per_state(fresh).items())
    graph = fresh.capture(keep_graph=True)
    cap = Captured(graph, torch.cuda.current_stream(), 'per.SAC.step')
    nodes = dict(cap.node_types())
    print('per.SAC.step graph:', nodes)
    launches = P.per_api().lib.eb_per_set_launches(300, X)
    assert fresh.KERNELS == O.SAC.KERNELS + 2 + launches == 47 and nodes == {'kernel': fresh.KERNELS} and cap.is_chain()
    assert all(bits(x, start[k]) for k, x in per_state(fresh).items())            # nothing ran during the capture
    fresh.replay(graph)
    once = per_state(fresh)
    for k, x in once.items():
        assert bits(x, eager[k]), k
    fresh.replay(graph)
    again = per_state(fresh)
    second = P.sample_reference(once['prio'], n, seed=5, draw=0, base=1)
    assert np.array_equal(again['index'], second['index']) and not np.array_equal(again['index'], once['index'])
    assert np.array_equal(again['tree'], P.tree_reference(again['prio'])) and again['counter'].tolist() == [2]
    assert fresh.log()['beta'] == float(P.beta_reference(0.4, 0.25, 1))
    sac.step()                                                                     # the eager twin of the second replay
    torch.cuda.synchronize()
    for k, x in per_state(sac).items():
        assert bits(x, again[k]), k


def test_the_uniform_sac_is_the_42_kernels_it_was():
    """offpolicy.SAC.step() was split into overridable pieces for per.SAC: its graph is still 42 kernel nodes in one chain"""
    import torch
    from tests.test_gpu_offpolicy import sac_setup
    sac, _ = sac_setup()
    cap = Captured(sac.capture(keep_graph=True), torch.cuda.current_stream(), 'SAC.step')
    assert dict(cap.node_types()) == {'kernel': 42} and cap.is_chain()


# ---- 7: the example -------------------------------------------------------------------------------------------------------------------------------
def test_sac_per_loop_example_runs():
    spec = importlib.util.spec_from_file_location('sac_per_loop', os.path.join(ROOT, 'examples', 'sac_per_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    logs = mod.main(['--iterations', '3', '--n-env', '64', '--warmup', '2', '--batch', '64', '--capacity', '1000', '--hidden', '64'])
    assert len(logs) == 3 and [round(log['beta'], 3) for log in logs] == [0.4, 0.7, 1.0]
    for log in logs:
        assert all(np.isfinite(v) for v in log.values()) and 0 < log['weight'] <= 1, log
