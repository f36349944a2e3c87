"""GPU (-m gpu): the epoch family (include/envbuild_epoch.h) — the keyed and the explicit gather against NumPy indexing and
torch.index_select bit for bit, eb_adv_stats against float64 NumPy, eb_ppo_log against its restatement, the counter, every entry on a side
stream and under capture, `PPOEpochs` against the parent's route written out (eager, keyed, captured, without an allocation, its log),
and the example."""
import ctypes as C
import functools
import importlib.util
import itertools
import os

import numpy as np
import pytest

from env_build_amd import epoch
from tests import _epoch as T
from tests._capture import Captured, capture, side_stream
from tests._helpers import ROOT
from tests._policy import SENTINEL, same
from tests._ppo import gpu

pytestmark = pytest.mark.gpu

SPANS = ((0, None), (3, 1), (1, 63), (0, 64), (64, 65), (97, 300))            # (offset, count); None: n_total


def spans(n_total):
    return [(o, n_total if c is None else c) for o, c in SPANS if o + (n_total if c is None else c) <= n_total]


@functools.lru_cache(maxsize=None)
def reference(n, seed, ep, base=0):
    return epoch.index_reference(n, seed, ep, base)


def sources_of(n_total, widths, seed=0):
    rng = np.random.default_rng(seed + n_total + sum(widths))
    return [rng.standard_normal((n_total, w)).astype(np.float32) for w in widths]


class Dests(object):
    """destinations of `count` rows cut from ONE buffer at odd float offsets, with sentinel gaps between them"""

    def __init__(self, count, widths, gap=3):
        import torch
        self.at, at = [], 1
        for w in widths:
            self.at.append(at)
            at += count * w + gap
            at += 1 - at % 2                                                 # the next one starts at an odd offset too
        self.count, self.widths = count, widths
        self.buf = torch.full((at + gap,), SENTINEL, device='cuda')
        self.views = [self.buf[a:a + count * w] for a, w in zip(self.at, widths)]

    def host(self):
        import torch
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        inside = np.zeros(raw.size, bool)
        out = []
        for a, w in zip(self.at, self.widths):
            inside[a:a + self.count * w] = True
            out.append(raw[a:a + self.count * w].reshape(self.count, w).copy())
        return out, bool((raw[~inside] == SENTINEL).all())


# ---- 1: the keyed route's indices ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_total', [1, 65, 257, 4097])
def test_keyed_gather_takes_the_rows_index_reference_names(n_total):
    import torch
    (src,) = sources_of(n_total, (1,))
    s = gpu(src)
    counters = {None: None, 0: torch.zeros(1, dtype=torch.int64, device='cuda'), 5: torch.full((1,), 5, dtype=torch.int64, device='cuda')}
    for offset, count in spans(n_total):
        dst = torch.full((count, 1), SENTINEL, device='cuda')
        index_out = torch.full((count,), -9, dtype=torch.int32, device='cuda')
        for seed, ep, base in itertools.product((0, 5), (0, 5), (None, 0, 5)):
            epoch.gather([s], [dst], offset, count, seed=seed, epoch=ep, counter=counters[base], index_out=index_out)
            want = reference(n_total, seed, ep, base or 0)[offset:offset + count]
            assert np.array_equal(index_out.cpu().numpy(), want), (n_total, offset, count, seed, ep, base)
            assert same(dst.cpu().numpy(), src[want])
    assert counters[5].item() == 5 and counters[0].item() == 0              # the gather only reads the counter


# ---- 2: gathered rows ------------------------------------------------------------------------------------------------------------------------
GATHER_CASES = [((41, 2, 1, 1, 1, 1), 257, 64, 65), ((41, 2, 1, 1, 1, 1), 4097, 97, 300), ((1,), 257, 1, 63), ((2,), 257, 64, 65), ((64,), 257, 0, 257),
                ((137,), 4097, 97, 300), ((137,), 65, 3, 1), ((41, 2, 1, 1, 1, 1, 3, 137), 257, 0, 257), ((2, 1, 2, 1, 2, 1, 2, 1), 65, 0, 65)]


@pytest.mark.parametrize('widths,n_total,offset,count', GATHER_CASES)
def test_gathered_rows_are_the_source_rows(widths, n_total, offset, count):
    import torch
    srcs = sources_of(n_total, widths)
    dev = [gpu(a) for a in srcs]
    dev = [d[:, 0].contiguous() if w == 1 and k % 2 else d for k, (d, w) in enumerate(zip(dev, widths))]      # [n] and [n, 1] both
    d = Dests(count, widths)
    index_out = torch.full((count,), -9, dtype=torch.int32, device='cuda')
    epoch.gather(dev, d.views, offset, count, seed=7, epoch=2, index_out=index_out)
    got, gaps_untouched = d.host()
    want = reference(n_total, 7, 2)[offset:offset + count]
    assert np.array_equal(index_out.cpu().numpy(), want)
    for k, (g, a) in enumerate(zip(got, srcs)):
        assert same(g, a[want]), (k, widths[k])
    assert gaps_untouched
    for t, a in zip(dev, srcs):
        assert same(t.cpu().numpy().reshape(a.shape), a)                      # the sources are not written


# ---- 3: the explicit route -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['int32', 'int64'])
def test_explicit_permutation_equals_index_select_and_a_bad_index_is_never_read(dtype):
    import torch
    widths, n_total, slack = (41, 2, 1, 1, 1, 1), 257, 2
    torch.manual_seed(3)
    perm = torch.randperm(n_total, device='cuda').to(getattr(torch, dtype))
    # the sources are views into the middle of larger allocations: `slack` rows of sentinels on both sides
    srcs = sources_of(n_total, widths)
    big = [torch.full((n_total + 2 * slack, w), SENTINEL, device='cuda') for w in widths]
    views = []
    for b, a in zip(big, srcs):
        b[slack:slack + n_total] = gpu(a)
        views.append(b[slack:slack + n_total])
    assert all(v.is_contiguous() and v.data_ptr() != b.data_ptr() for v, b in zip(views, big))
    for offset, count in ((0, n_total), (64, 65), (3, 1)):
        d = Dests(count, widths)
        index_out = torch.full((count,), -9, dtype=torch.int32, device='cuda')
        epoch.gather(views, d.views, offset, count, perm=perm, index_out=index_out)
        got, gaps_untouched = d.host()
        idx = perm[offset:offset + count].long()
        for g, v, w in zip(got, views, widths):
            want = torch.empty((count, w), device='cuda')
            torch.index_select(v, 0, idx, out=want)
            assert same(g, want.cpu().numpy())
        assert gaps_untouched and np.array_equal(index_out.cpu().numpy(), idx.cpu().numpy())
    # -1 and n_total planted at two positions: those rows are quiet NaNs in every source, index_out -1, the other rows right
    bad = perm.clone()
    bad[5], bad[70] = -1, n_total
    d = Dests(n_total, widths)
    index_out = torch.full((n_total,), -9, dtype=torch.int32, device='cuda')
    epoch.gather(views, d.views, 0, n_total, perm=bad, index_out=index_out)
    got, gaps_untouched = d.host()
    idx = perm.cpu().numpy().astype(np.int64)
    ok = np.ones(n_total, bool)
    ok[[5, 70]] = False
    for g, a in zip(got, srcs):
        assert np.isnan(g[~ok]).all() and (g[~ok].view(np.uint32) == 0x7FC00000).all()
        assert same(g[ok], a[idx[ok]])
    io = index_out.cpu().numpy()
    assert gaps_untouched and (io[~ok] == -1).all() and np.array_equal(io[ok], idx[ok])
    for b, a in zip(big, srcs):                                               # sources and their slack are as made
        raw = b.cpu().numpy()
        assert same(raw[slack:slack + n_total], a) and (raw[:slack] == SENTINEL).all() and (raw[slack + n_total:] == SENTINEL).all()


def test_gather_refusals_write_nothing():
    import torch
    src, dst = torch.zeros((16, 3), device='cuda'), torch.full((4, 3), SENTINEL, device='cuda')
    api = epoch.epoch_api()

    def call(**kw):
        a = epoch.EbGatherArgs(n_total=16, offset=0, count=4, n_sources=1)
        a.sources[0].src, a.sources[0].dst, a.sources[0].width = src.data_ptr(), dst.data_ptr(), 3
        for k, v in kw.items():
            setattr(a, k, v)
        return api.minibatch_gather(C.byref(a))

    with pytest.raises(ValueError, match='eb_minibatch_gather'):
        api.check(call(offset=13))
    assert call(n_sources=9) == -1 and call(perm=src.data_ptr(), perm_bytes=3) == -1 and call(count=2 ** 31) == -1
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()
    with pytest.raises(TypeError):
        epoch.gather([src.cpu()], [dst], 0, 4)                               # there is no CPU path


# ---- 4: the statistics ----------------------------------------------------------------------------------------------------------------------
def stats_input(n):
    rng = np.random.default_rng(n)
    return (0.7 + 1.9 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize('n', [2, 63, 64, 65, 1025, 100003])
def test_adv_stats_against_float64_numpy(n):
    import torch
    x = stats_input(n)
    out, std_out = torch.full((2,), SENTINEL, device='cuda'), torch.full((1,), SENTINEL, device='cuda')
    assert epoch.adv_stats(gpu(x), 1e-8, out=out, std_out=std_out) is out
    mean, inv = out.cpu().numpy()
    std = std_out.cpu().numpy()[0]
    x64 = x.astype(np.float64)
    want_mean, want_std = np.float32(np.mean(x64)), np.float32(np.std(x64, ddof=1))
    print('n %d: mean %r (float64 rounded: %r), std %r (%r)' % (n, mean, want_mean, std, want_std))
    assert abs(float(mean) - float(want_mean)) <= float(np.spacing(np.abs(want_mean)))
    assert abs(float(std) - float(want_std)) <= float(np.spacing(want_std))
    assert inv == np.float32(1.0) / (std + np.float32(1e-8))                 # bit for bit, of its own std
    ref = epoch.adv_stats_reference(x, 1e-8, np.float32)
    assert (mean, inv, std) == ref                                            # the restatement's order is the kernels'
    got = epoch.adv_stats(gpu(x))                                             # allocates its outputs
    assert same(got.cpu().numpy(), np.array([mean, inv], np.float32))


def test_adv_stats_feeds_the_surrogate_a_nan_travels_and_a_refusal_writes_nothing():
    import torch
    from env_build_amd import train
    surr = []
    for route in ('entry', 'copied', 'unnormalised'):
        policy, value = T.make_nets()
        upd = train.PPOUpdate(policy, value, T.N, **T.PPO_KW)
        data = T.make_data(policy)
        for k in T.FIELDS:
            getattr(upd.mb, k).copy_(data[k])
        if route == 'entry':
            epoch.adv_stats(data['adv'], 1e-8, out=upd.mb.adv_norm)          # written where the surrogate reads it
            norm = upd.mb.adv_norm.cpu().numpy().copy()
        elif route == 'copied':
            upd.mb.adv_norm.copy_(gpu(norm))
        upd.step()
        surr.append(T.snapshot(upd)['surr'])
    adv = data['adv'].cpu().numpy().astype(np.float64)
    assert abs(norm[0] - np.mean(adv)) <= 1e-6 and abs(norm[1] - 1.0 / np.std(adv, ddof=1)) <= 1e-6
    assert same(surr[0], surr[1]) and not same(surr[0], surr[2])
    # a NaN travels
    x = stats_input(1025)
    x[1000] = np.nan
    out, std_out = torch.zeros(2, device='cuda'), torch.zeros(1, device='cuda')
    epoch.adv_stats(gpu(x), out=out, std_out=std_out)
    assert torch.isnan(out).all() and torch.isnan(std_out).all()
    # n = 1 is refused by name and writes nothing
    out.fill_(SENTINEL)
    with pytest.raises(ValueError, match='eb_adv_stats'):
        epoch.adv_stats(gpu(x[:1]), out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- 5: the log -------------------------------------------------------------------------------------------------------------------------------
def log_inputs(n):
    rng = np.random.default_rng(n)
    logp_old = (-1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    logp = (logp_old + 0.1 * rng.standard_normal(n)).astype(np.float32)
    ratio = np.exp(logp - logp_old).astype(np.float32)
    return dict(logp=logp, logp_old=logp_old, ratio=ratio, surr=(ratio * rng.standard_normal(n)).astype(np.float32),
                ent=(1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32), vloss=(0.5 * rng.standard_normal(n) ** 2).astype(np.float32))


def run_log(x, clip, out=None):
    import torch
    dev = {k: None if v is None else gpu(v) for k, v in x.items()}
    out = torch.full((64, 8), SENTINEL, dtype=torch.float64, device='cuda') if out is None else out
    epoch.ppo_log({k: v for k, v in dev.items() if k != 'logp_old'}, dev['logp_old'], clip, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def held_to_reference(got, x, clip):
    want = epoch.ppo_log_reference(clip=clip, **x)
    for f in (3, 5, 6, 7):                                                    # counts, the maximum and the row counts: exact
        assert np.array_equal(got[:, f], want[:, f]), f
    sums = {0: x['surr'], 1: x['vloss'], 2: x['ent'], 4: None if x['logp'] is None or x['logp_old'] is None else x['logp_old'] - x['logp']}
    for f, a in sums.items():
        bar = 0.0 if a is None else 1e-12 * np.abs(np.where(np.isfinite(a), a, 0.0)).sum(dtype=np.float64)
        finite = np.isfinite(want[:, f])
        assert np.array_equal(np.isfinite(got[:, f]), finite), f
        assert (np.abs(got[finite, f] - want[finite, f]) <= bar).all(), (f, np.abs(got[finite, f] - want[finite, f]).max(), bar)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 16385])
def test_ppo_log_blocks_equal_the_restatement(n):
    x = log_inputs(n)
    got = run_log(x, 0.2)
    held_to_reference(got, x, 0.2)
    assert got[:, 7].sum() == n and (got[(n + 255) // 256:] == 0.0).all()    # blocks without rows write zeros
    if n == 16385:
        assert got[0, 7] == 257.0                                             # block 0 took the row 16384 in its second round
    folded = epoch.fold_log(got)
    assert folded['rows'] == n and folded['max_ratio_dev'] == np.abs(x['ratio'] - np.float32(1.0)).max()
    assert folded['clip_fraction'] * n == (np.abs(x['ratio'] - np.float32(1.0)) > np.float32(0.2)).sum()


def test_ppo_log_with_each_input_missing_and_with_bad_rows():
    n = 600
    x = log_inputs(n)
    for gone in x:
        part = dict(x)
        part[gone] = None
        held_to_reference(run_log(part, 0.1), part, 0.1)
    x['ratio'][5], x['surr'][300], x['logp'][300], x['ent'][599] = np.nan, np.inf, -np.inf, np.nan
    got = run_log(x, 0.2)
    held_to_reference(got, x, 0.2)
    assert got[:, 6].sum() == 3 and np.isfinite(got[:, 5]).all() and np.isinf(got[1, 0]) and np.isnan(got[2, 2])


# ---- 6: the counter -----------------------------------------------------------------------------------------------------------------------------
def advance(counter, by, stream=None):
    api = epoch.epoch_api()
    api.check(api.epoch_advance(C.byref(epoch.EbEpochAdvanceArgs(counter=counter.data_ptr(), by=by, stream=stream))))


def test_epoch_advance_adds():
    import torch
    counter = torch.tensor([7, -77], dtype=torch.int64, device='cuda')
    advance(counter, 4)
    advance(counter, 4)
    assert counter.cpu().tolist() == [15, -77]
    advance(counter, 2 ** 40)
    assert counter.cpu().tolist() == [15 + 2 ** 40, -77]


# ---- 7: streams and capture ------------------------------------------------------------------------------------------------------------------
def test_every_entry_on_a_side_stream_and_under_capture():
    import torch
    api = epoch.epoch_api()
    side = side_stream()
    n_total, widths, count = 257, (41, 2, 1), 65
    srcs = [gpu(a) for a in sources_of(n_total, widths)]
    x = stats_input(1025)
    xd = gpu(x)
    lg = {k: gpu(v) for k, v in log_inputs(300).items()}
    outs = dict(g0=torch.empty((count, 41), device='cuda'), g1=torch.empty((count, 2), device='cuda'), g2=torch.empty((count, 1), device='cuda'),
                index=torch.empty((count,), dtype=torch.int32, device='cuda'), norm=torch.empty((2,), device='cuda'),
                log=torch.empty((64, 8), dtype=torch.float64, device='cuda'), counter=torch.zeros((1,), dtype=torch.int64, device='cuda'))
    partials = torch.zeros(512, dtype=torch.float64, device='cuda')
    base = torch.full((1,), 2, dtype=torch.int64, device='cuda')

    def run_gather(s):
        a = epoch._gather_args(srcs, [outs['g0'], outs['g1'], outs['g2']], 64, count, None, 9, 1, base, outs['index'])
        a.stream = s
        api.check(api.minibatch_gather(C.byref(a)))

    def run_stats(s):
        a = epoch.EbAdvStatsArgs(n=1025, x=xd.data_ptr(), eps=1e-8, out=outs['norm'].data_ptr(), partials=partials.data_ptr(), stream=s)
        api.check(api.adv_stats(C.byref(a)))

    def run_log_(s):
        a = epoch._log_args({k: v for k, v in lg.items() if k != 'logp_old'}, lg['logp_old'], 0.2, outs['log'])
        a.stream = s
        api.check(api.ppo_log(C.byref(a)))

    def run_advance(s):
        advance(outs['counter'], 3, s)

    entries = (('eb_minibatch_gather', run_gather, ('g0', 'g1', 'g2', 'index'), 1), ('eb_adv_stats', run_stats, ('norm',), 2),
               ('eb_ppo_log', run_log_, ('log',), 1), ('eb_epoch_advance', run_advance, ('counter',), 1))

    def poison(names):
        for k in names:
            outs[k].fill_(0 if k == 'counter' else -77)
        torch.cuda.synchronize()

    def snap(names):
        torch.cuda.synchronize()
        return {k: outs[k].cpu().numpy().copy() for k in names}

    for name, run, names, kernels in entries:
        poison(names)
        run(None)
        want = snap(names)
        poisoned = {k: np.full_like(v, 0 if k == 'counter' else -77) for k, v in want.items()}
        assert not any(same(want[k], poisoned[k]) for k in names), name
        poison(names)
        run(side.cuda_stream)
        assert all(same(v, want[k]) for k, v in snap(names).items()), name
        poison(names)
        cap = capture(side, run, name)
        try:
            assert all(same(v, poisoned[k]) for k, v in snap(names).items()), '%s ran under capture' % name
            nodes = dict(cap.node_types())
            print('%s:' % name, nodes)
            assert nodes == {'kernel': kernels} and cap.is_chain(), name      # no memset, no memcpy
            for _ in range(2):
                poison(names)
                cap.replay()
                assert all(same(v, want[k]) for k, v in snap(names).items()), name
        finally:
            cap.close()
    assert same(outs['index'].cpu().numpy().astype(np.int64), reference(n_total, 9, 1, 2)[64:64 + count])


# ---- 8: PPOEpochs ------------------------------------------------------------------------------------------------------------------------------
def parent_route(perm, per_minibatch=None):
    """the parent's update phase written out: adv_norm once, then per epoch and minibatch six index_selects with the slice of that epoch's
    permutation and PPOUpdate.step() -> (the update, its data).  per_minibatch(upd) is called after every step."""
    import torch
    from env_build_amd import train
    policy, value = T.make_nets()
    upd = train.PPOUpdate(policy, value, T.ROWS, **T.PPO_KW)
    data = T.make_data(policy)
    epoch.adv_stats(data['adv'], 1e-8, out=upd.mb.adv_norm)
    for e in range(T.EPOCHS):
        for k in range(T.MINIBATCHES):
            idx = perm[e][k * T.ROWS:(k + 1) * T.ROWS]
            for name in T.FIELDS:
                torch.index_select(data[name], 0, idx, out=getattr(upd.mb, name))
            upd.step()
            if per_minibatch is not None:
                per_minibatch(upd)
    return upd, data


def epochs_of(**kw):
    from env_build_amd import train
    policy, value = T.make_nets()
    upd = train.PPOUpdate(policy, value, T.ROWS, **T.PPO_KW)
    data = T.make_data(policy)
    return epoch.PPOEpochs(upd, data, T.EPOCHS, T.MINIBATCHES, **kw), upd, data


def keyed_perm(base=0):
    import torch
    return torch.from_numpy(np.stack([epoch.index_reference(T.N, T.SEED, e, base) for e in range(T.EPOCHS)])).cuda()


def differing(a, b):
    return [k for k in a if not same(a[k], b[k])]


@pytest.fixture(scope='module')
def parent():
    """the parent's route fed the keyed permutations of iteration 0, with rows.* and mb.logp_old snapshotted per minibatch; and of
    iterations 0 and 1 in a row.  Computed once, left unchanged."""
    import torch
    per = []

    def keep(upd):
        torch.cuda.synchronize()
        rows = {k: getattr(upd.rows, k).cpu().numpy().copy() for k in ('logp', 'ratio', 'surr', 'ent', 'vloss')}
        per.append(dict(rows, logp_old=upd.mb.logp_old.cpu().numpy().copy()))

    upd, _ = parent_route(keyed_perm(0), keep)
    return dict(final=T.snapshot(upd), per=per)


def test_ppo_epochs_with_a_given_permutation_equals_the_parents_route(parent):
    import torch
    perm = keyed_perm(0)
    for dtype in (torch.int64, torch.int32):
        loop, upd, _ = epochs_of(perm=perm.to(dtype), keep_index=True)
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_stats()['allocation.all.allocated']
        loop.step()
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == allocated      # no allocation across a step
        got = T.snapshot(upd)
        assert not differing(parent['final'], got), differing(parent['final'], got)
        assert got['state'][0] == T.EPOCHS * T.MINIBATCHES
        want = perm.cpu().numpy()[:, :T.MINIBATCHES * T.ROWS].reshape(T.EPOCHS, T.MINIBATCHES, T.ROWS)
        assert np.array_equal(loop.index.cpu().numpy(), want)
        assert loop.counter.item() == T.EPOCHS


def test_ppo_epochs_keyed_route_and_its_log(parent):
    import torch
    loop, upd, _ = epochs_of(seed=T.SEED)
    loop.step()
    got = T.snapshot(upd)
    assert not differing(parent['final'], got), differing(parent['final'], got)
    # the log: fold_log of the restatement on rows.* as they were after every minibatch of the parent's route
    log = loop.log()
    clip = np.float32(T.PPO_KW['clip'])
    for e in range(T.EPOCHS):
        for k in range(T.MINIBATCHES):
            rows = parent['per'][e * T.MINIBATCHES + k]
            want = epoch.fold_log(epoch.ppo_log_reference(clip=clip, **rows))
            for name in ('clip_fraction', 'max_ratio_dev', 'nonfinite_rows', 'rows'):
                assert log[name][e, k] == want[name], (name, e, k)
            sums = dict(policy_loss=rows['surr'], value_loss=rows['vloss'], entropy=rows['ent'], approx_kl=rows['logp_old'] - rows['logp'])
            for name, a in sums.items():
                assert abs(log[name][e, k] - want[name]) <= 1e-12 * np.abs(a).sum(dtype=np.float64) / T.ROWS, (name, e, k)
    assert all(v.shape == (T.EPOCHS, T.MINIBATCHES) for v in log.values())
    assert log['max_ratio_dev'][0, 0] == 0.0 and log['approx_kl'][0, 0] == 0.0          # the first pass: ratio exactly 1
    assert (log['max_ratio_dev'].ravel()[1:] > 0.0).all() and (log['nonfinite_rows'] == 0).all() and (log['rows'] == T.ROWS).all()


def test_ppo_epochs_two_replays_equal_two_eager_steps():
    import torch
    from env_build_amd import ppo
    eager, upd_e, _ = epochs_of(seed=T.SEED, keep_index=True)
    eager.step()
    first = T.snapshot(upd_e)
    first_index = eager.index.cpu().numpy().copy()
    eager.step()
    second = T.snapshot(upd_e)
    second_index, second_log = eager.index.cpu().numpy().copy(), eager.log()
    assert np.array_equal(second_index.reshape(T.EPOCHS, -1), keyed_perm(T.EPOCHS).cpu().numpy()[:, :T.MINIBATCHES * T.ROWS])
    assert not np.array_equal(first_index, second_index) and differing(first, second)
    # captured
    loop, upd, data = epochs_of(seed=T.SEED, keep_index=True)
    before = T.snapshot(upd)
    graph = loop.capture(keep_graph=True)
    during = T.snapshot(upd)
    assert not differing(before, during) and loop.counter.item() == 0, 'the chain ran under capture'
    seen = Captured(graph, torch.cuda.current_stream(), 'PPOEpochs.step')
    nodes = dict(seen.node_types())
    print('PPOEpochs.step:', nodes)
    assert nodes == {'kernel': 3 + 15 * T.EPOCHS * T.MINIBATCHES} and seen.is_chain()
    stale, _ = ppo.policy_loss(upd.policy, data['obs'].cpu().numpy(), data['actions'].cpu().numpy(), data['logp_old'],
                               data['adv'].cpu().numpy(), 1.0, 0.2, 1e-3)             # an autograd graph built before the replay
    version = upd.policy._flat._version
    loop.replay(graph)
    assert upd.policy._flat._version > version and upd.policy._uploaded == upd.policy._flat._version
    assert upd.value._uploaded == upd.value._flat._version
    with pytest.raises(RuntimeError, match='modified in place'):
        stale.backward()
    got = T.snapshot(upd)
    assert not differing(first, got), differing(first, got)
    assert np.array_equal(loop.index.cpu().numpy(), first_index) and loop.counter.item() == T.EPOCHS
    loop.replay(graph)
    got = T.snapshot(upd)
    assert not differing(second, got), differing(second, got)
    assert np.array_equal(loop.index.cpu().numpy(), second_index) and loop.counter.item() == 2 * T.EPOCHS
    assert got['state'][0] == 2 * T.EPOCHS * T.MINIBATCHES
    log = loop.log()
    assert all(np.array_equal(log[k], second_log[k]) for k in log)
    torch.cuda.synchronize()
    graph.reset()


def test_ppo_epochs_refuses_what_it_cannot_run():
    import torch
    from env_build_amd import train
    policy, value = T.make_nets()
    upd = train.PPOUpdate(policy, value, T.ROWS, **T.PPO_KW)
    data = T.make_data(policy)
    with pytest.raises(ValueError, match='minibatches'):
        epoch.PPOEpochs(upd, data, 2, 5)
    with pytest.raises(ValueError, match='lacks'):
        epoch.PPOEpochs(upd, {k: v for k, v in data.items() if k != 'ret'}, 2, 4)
    with pytest.raises(TypeError):
        epoch.PPOEpochs(upd, data, 2, 4, perm=torch.zeros((2, T.N), device='cuda'))
    with pytest.raises(TypeError):
        epoch.PPOEpochs(upd, dict(data, adv=data['adv'].cpu()), 2, 4)


# ---- 9: the example ---------------------------------------------------------------------------------------------------------------------------
def test_ppo_epoch_loop_example_runs():
    spec = importlib.util.spec_from_file_location('ppo_epoch_loop', os.path.join(ROOT, 'examples', 'ppo_epoch_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(n_env=256, steps=8, epochs=2, minibatches=2, num_hidden_units=64)
    log = res['log']
    for name in ('policy_loss', 'value_loss', 'entropy', 'clip_fraction', 'approx_kl', 'max_ratio_dev'):
        assert log[name].shape == (2, 2) and np.isfinite(log[name]).all(), name
    assert (log['nonfinite_rows'] == 0).all() and (log['rows'] == 1024).all()
    assert res['policy_delta'] > 0.0 and res['value_delta'] > 0.0
    assert res['optimiser_steps'] == 4 and res['counter'] == 2
    assert log['max_ratio_dev'][0, 0] == 0.0 and log['approx_kl'][0, 0] == 0.0
