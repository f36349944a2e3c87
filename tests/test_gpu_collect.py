"""GPU (-m gpu): the collection family (include/envbuild_collect.h) — eb_collect_begin and eb_collect_record against `record_reference` bit
for bit on synthetic steps, eb_collect_next_values, eb_collect_episode_log against its restatement, every entry on a side stream and
under capture, `Collector` against the parent's collection and head written out, and the example."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from env_build_amd import collect
from tests import _collect as T
from tests._capture import capture, side_stream
from tests._helpers import ROOT
from tests._policy import same
from tests._ppo import gpu

pytestmark = pytest.mark.gpu

STEPS = 3


def dev_u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).cuda()


# ---- 1: begin and record on synthetic steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_final', [True, False])
@pytest.mark.parametrize('D', [1, 41, 137])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 257])
def test_begin_and_record_equal_the_restatement(B, D, with_final):
    """T = 3, two iterations in a row on one buffer.  B * D is a multiple of 4 at (64, 41), (64, 137) ...: every slot on the 16-byte
    path when the buffer starts aligned (slack 4 floats); otherwise the odd slots go as dwords; with slack 3 nothing is aligned."""
    import torch
    slack = 4 if with_final else 3
    want = T.sentinel_buffers(STEPS, B, D)
    got = T.Slack(T.sentinel_buffers(STEPS, B, D), slack)
    seen, ever = set(), np.zeros(B, bool)
    for iteration in range(2):
        first = np.random.default_rng(B + D + iteration).standard_normal((B, D)).astype(np.float32)
        first_d = gpu(first)
        collect.begin(first_d, got.views['obs_buf'], got.views['trunc_t'])
        collect.begin_reference(want, first)
        inputs = []
        for t in range(STEPS):
            obs, reward, code, final = T.step_inputs(B, D, t, iteration)
            dev = (gpu(obs), gpu(reward), dev_u8(code), gpu(final) if with_final else None)
            collect.record(t, dev[0], dev[1], dev[2], dev[3], got.views)
            collect.record_reference(want, t, obs, reward, code, final if with_final else None)
            inputs.append((dev, (obs, reward, code, final)))
            seen |= set(code.tolist())
        have, slack_untouched = got.host()
        for k in want:
            assert have[k].dtype == want[k].dtype and same(have[k], want[k]), (k, iteration)
        assert slack_untouched, iteration
        ever |= want['trunc_t'] >= 0                                          # (begin resets trunc_t, not the rows of the iteration before)
        assert (have['trunc_obs'][~ever] == T.SENTINEL).all()                # rows of envs that were never truncated keep their sentinel
        assert same(first_d.cpu().numpy(), first)
        for dev, host in inputs:                                              # the inputs are unchanged
            for d, h in zip(dev, host):
                assert d is None or same(d.cpu().numpy(), h)
    assert {0, 7} <= seen and (B < 8 or seen == set(range(8)))
    if with_final:
        assert (want['trunc_t'] >= 0).any()
    else:
        assert (want['trunc_t'] == -1).all() and (want['trunc_obs'] == T.SENTINEL).all()
    assert want['ep_len'].max() > 0 or B == 1                                 # the state carried across the two iterations
    torch.cuda.synchronize()


def test_record_refusals_write_nothing():
    import torch
    B, D = 5, 3
    got = T.Slack(T.sentinel_buffers(STEPS, B, D), 4)
    obs, reward, code, final = (gpu(a) if a.dtype == np.float32 else dev_u8(a) for a in T.step_inputs(B, D, 0, 0))
    with pytest.raises(ValueError, match='eb_collect_record'):
        collect.record(STEPS, obs, reward, code, final, got.views)
    with pytest.raises(ValueError, match='eb_collect_record'):
        collect.record(-1, obs, reward, code, None, got.views)
    have, slack_untouched = got.host()
    want = T.sentinel_buffers(STEPS, B, D)
    assert slack_untouched and all(same(have[k], want[k]) for k in want)
    with pytest.raises(TypeError):
        collect.record(0, obs.cpu(), reward, code, final, got.views)         # there is no CPU path
    with pytest.raises(TypeError):
        collect.begin(obs.cpu(), got.views['obs_buf'], got.views['trunc_t'])
    torch.cuda.synchronize()


# ---- 2: the bootstrap values ---------------------------------------------------------------------------------------------------------------------
def next_values_case(Tn, B):
    rng = np.random.default_rng(10 * Tn + B)
    values = rng.standard_normal((Tn + 1, B)).astype(np.float32)
    trunc_t = rng.choice(np.array([-1, 0, Tn - 1], np.int32), B).astype(np.int32)
    trunc_t[0] = Tn - 1 if B == 1 else -1
    if B > 1:
        trunc_t[1] = 0
    v_trunc = rng.standard_normal(B).astype(np.float32)
    v_trunc[trunc_t < 0] = np.nan                                            # unused rows: their NaN must not travel
    return values, v_trunc, trunc_t


@pytest.mark.parametrize('Tn', [1, 3])
@pytest.mark.parametrize('B', [1, 65])
def test_next_values_is_a_select(B, Tn):
    values, v_trunc, trunc_t = next_values_case(Tn, B)
    arrays = dict(values=values, v_trunc=v_trunc, trunc_t=trunc_t, out=np.full((Tn, B), T.SENTINEL, np.float32))
    d = T.Slack(arrays, 3)
    assert collect.next_values(d.views['values'], d.views['v_trunc'], d.views['trunc_t'], d.views['out']) is d.views['out']
    have, slack_untouched = d.host()
    want = collect.next_values_reference(values, v_trunc, trunc_t)
    assert same(have['out'], want) and slack_untouched and not np.isnan(have['out']).any()
    assert (trunc_t >= 0).any() and (B == 1 or np.isnan(v_trunc).any())
    for k in ('values', 'v_trunc', 'trunc_t'):
        assert same(have[k], arrays[k]), k


# ---- 3: the episode log ---------------------------------------------------------------------------------------------------------------------------
def log_inputs(n):
    rng = np.random.default_rng(n)
    ret = (3.0 + 20.0 * rng.standard_normal(n)).astype(np.float32)
    length = rng.integers(1, 200, n).astype(np.int32)
    code = (rng.integers(0, 8, n) * (rng.random(n) < 0.5)).astype(np.uint8)
    code[0] = 6
    if n >= 255:
        code[[3, 77, 200]] = (1, 7, 2)
        ret[3], ret[77] = np.nan, np.inf
        ret[200] = -np.inf
    return ret, length, code


def held_to_reference(got, ret, length, code):
    """DESIGN.md §25's bars for the same fold: counts, maximum and minimum exact, sums within 1e-12 of sum |x|"""
    want = collect.episode_log_reference(ret, length, code)
    for f in (0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert np.array_equal(got[:, f], want[:, f]), f
    done = (code != 0) & np.isfinite(ret)
    R = np.where(done, ret, 0).astype(np.float64)
    bars = {1: np.abs(R).sum(), 2: (R * R).sum(), 3: np.where(code != 0, length, 0).astype(np.float64).sum()}
    for f, scale in bars.items():
        finite = np.isfinite(want[:, f])
        assert np.array_equal(np.isfinite(got[:, f]), finite) and same(got[~finite, f], want[~finite, f]), f
        assert (np.abs(got[finite, f] - want[finite, f]) <= 1e-12 * scale).all(), (f, np.abs(got[finite, f] - want[finite, f]).max())


@pytest.mark.parametrize('n', [1, 255, 256, 257, 16385])
def test_episode_log_blocks_equal_the_restatement(n):
    import torch
    ret, length, code = log_inputs(n)
    out = torch.full((64, 16), T.SENTINEL, dtype=torch.float64, device='cuda')
    assert collect.episode_log(gpu(ret), torch.from_numpy(length).cuda(), dev_u8(code), out) is out
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    held_to_reference(got, ret, length, code)
    assert got[:, 15].sum() == n
    empty = got[:, 15] == 0
    assert empty.sum() == max(0, 64 - (n + 255) // 256)
    assert (got[empty][:, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]] == 0.0).all()     # blocks without slots write zeros,
    assert (got[empty, 4] == -np.inf).all() and (got[empty, 5] == np.inf).all()                 # the maximum and minimum at their neutral values
    if n == 16385:
        assert got[0, 15] == 257.0                                            # block 0 took the slot 16384 in its second round
    folded = collect.fold_episode_log(got)
    assert folded['slots'] == n and folded['episodes'] == int((code != 0).sum()) and folded['nonfinite'] == (3 if n >= 255 else 0)
    assert folded['outcomes']['good_done'] == int((code == 6).sum()) and sum(folded['outcomes'].values()) == n


# ---- 4: streams and capture -----------------------------------------------------------------------------------------------------------------------
def test_every_entry_on_a_side_stream_and_under_capture():
    import torch
    api = collect.collect_api()
    side = side_stream()
    B, D = 65, 41
    buf = collect.buffers(STEPS, B, D, 'cuda')
    first = gpu(np.random.default_rng(1).standard_normal((B, D)))
    obs, reward, code, final = (gpu(a) if a.dtype == np.float32 else dev_u8(a) for a in T.step_inputs(B, D, 1, 0))
    values, v_trunc, trunc_t = next_values_case(STEPS, B)
    nv_in = (gpu(values), gpu(np.nan_to_num(v_trunc)), torch.from_numpy(trunc_t).cuda())
    ret, length, cd = log_inputs(300)
    lg_in = (gpu(ret), torch.from_numpy(length).cuda(), dev_u8(cd))
    outs = dict(buf, nv=torch.empty((STEPS, B), device='cuda'), log=torch.empty((64, 16), dtype=torch.float64, device='cuda'))
    state = ('ep_ret', 'ep_len')

    def run_begin(s):
        a = collect._begin_args(first, buf['obs_buf'], buf['trunc_t'])
        a.stream = s
        api.check(api.begin(C.byref(a)))

    def run_record(s):
        a = collect._record_args(1, buf, obs, reward, code, final)
        a.stream = s
        api.check(api.record(C.byref(a)))

    def run_next(s):
        a = collect._next_values_args(nv_in[0], nv_in[1], nv_in[2], outs['nv'])
        a.stream = s
        api.check(api.next_values(C.byref(a)))

    def run_log(s):
        a = collect._episode_log_args(lg_in[0], lg_in[1], lg_in[2], outs['log'])
        a.stream = s
        api.check(api.episode_log(C.byref(a)))

    written = ('obs_buf', 'rew_buf', 'nonterminal', 'carry', 'ret_buf', 'len_buf', 'code_buf', 'trunc_obs', 'trunc_t', 'ep_ret', 'ep_len')
    entries = (('eb_collect_begin', run_begin, ('obs_buf', 'trunc_t')), ('eb_collect_record', run_record, written),
               ('eb_collect_next_values', run_next, ('nv',)), ('eb_collect_episode_log', run_log, ('log',)))

    def poison(names):
        for k in names:
            outs[k].fill_(3 if k in state else 99)                            # (the running state is an input too: the same start every time)
        torch.cuda.synchronize()

    def snap(names):
        torch.cuda.synchronize()
        return {k: outs[k].cpu().numpy().copy() for k in names}

    for name, run, names in entries:
        poison(names)
        poisoned = snap(names)
        run(None)
        want = snap(names)
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
            assert nodes == {'kernel': 1} and cap.is_chain(), name           # no memset, no memcpy
            for _ in range(2):
                poison(names)
                cap.replay()
                assert all(same(v, want[k]) for k, v in snap(names).items()), name
        finally:
            cap.close()


# ---- 5: the Collector ---------------------------------------------------------------------------------------------------------------------------
GAMMA, LAM, ENV_SEED = 0.99, 0.95, 0


def make_env(limit=5):
    from env_build_amd.endtoend import CrossroadEnd2end
    env = CrossroadEnd2end('left', n_env=65, auto_reset=True, copy_outputs=False, max_episode_steps=limit)
    env.seed(ENV_SEED)
    env.reset()
    env.reset()
    return env


def collector_nets(env):
    """tests/_epoch.make_nets with the example's observation scale on both networks and the value head's weights times 0.1 under its bias
    of at least 1: the relu is alive on the env's own observations, so a bootstrap from V(final observation) is a number that shows"""
    from tests import _epoch as E
    policy, value = E.make_nets()
    scale = [0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num
    w = value.get_weights()
    w[-2] = (w[-2] * np.float32(0.1)).astype(np.float32)
    value.set_weights(w)
    policy.set_obs_scale(scale)
    value.set_obs_scale(scale)
    return policy, value


def test_collector_equals_the_parents_route():
    """two envs under one seed, 41 -> 64 -> 64 -> 4 | 1 networks with the same weights; one driven by examples/ppo_epoch_loop.py's loop
    written out, the other by Collector(steps = 5 = the time limit); two iterations"""
    import torch
    from env_build_amd import ppo
    from env_build_amd.policy_logp import log_prob_actions
    Tn, B, seed = 5, 65, 11
    env_p, env_c = make_env(), make_env()
    D = env_p.obs_dim
    policy_p, value_p = collector_nets(env_p)
    policy_c, value_c = collector_nets(env_c)
    col = collect.Collector(env_c, policy_c, value_c, Tn, 1.0, seed=seed)
    truncated = live_slots = bootstrapped = 0
    for iteration in range(2):
        # the parent: collection, then the head of ppo_epoch_loop.py
        p = T.parent_collect(env_p, policy_p, Tn, seed, iteration)
        obs_all, act_all = p['obs'].view(Tn * B, D), p['act'].view(Tn * B, 2)
        with torch.no_grad():
            v = value_p(obs_all)[:, 0].view(Tn, B).contiguous()
            v_last = value_p(p['last'])[:, 0].contiguous()
            v_final = value_p(p['final'].view(Tn * B, D))[:, 0].view(Tn, B)
        live, trunc = p['code'] == 0, p['code'] == collect.TIME_LIMIT
        plain_adv, _ = ppo.gae(p['rew'], v, v_last, live.float(), GAMMA, LAM)
        nv = torch.where(trunc, v_final, torch.cat([v[1:], v_last[None]], 0)).contiguous()
        want_adv, want_ret = ppo.gae(p['rew'], v, None, (live | trunc).float(), GAMMA, LAM, next_values=nv, carry=live.float())
        want_logp = log_prob_actions(policy_p, obs_all, act_all, 1.0)['logp'].t
        # the Collector
        torch.cuda.synchronize()
        allocated = torch.cuda.memory_stats()['allocation.all.allocated']
        col.collect()
        data = col.finish(GAMMA, LAM)
        assert torch.cuda.memory_stats()['allocation.all.allocated'] == allocated, iteration      # no allocation
        torch.cuda.synchronize()
        host = lambda t: t.detach().cpu().numpy()
        assert same(host(data['obs']), host(obs_all)) and same(host(data['actions']), host(act_all)), iteration
        assert same(host(col.buf['rew_buf']), host(p['rew'])) and same(host(col.buf['code_buf']), host(p['code'])), iteration
        assert same(host(col.buf['obs_buf'][Tn]), host(p['last'])), iteration
        assert same(host(data['logp_old']), host(want_logp)), iteration
        assert same(host(col.values[:Tn]), host(v)) and same(host(col.values[Tn]), host(v_last)), iteration
        assert same(host(data['v_old']), host(v).reshape(-1)), iteration
        assert same(host(col.next_values), host(nv)), iteration
        assert same(host(data['adv']), host(want_adv.t).reshape(-1)) and same(host(data['ret']), host(want_ret.t).reshape(-1)), iteration
        # slots with no truncation in their env's future within the collection: the parent's plain gae says the same
        tr = host(trunc)
        clear = ~(np.cumsum(tr[::-1], axis=0)[::-1] > 0)
        assert same(host(col.adv)[clear], host(plain_adv.t)[clear]), iteration
        # ... and at a truncated step the bootstrap shows wherever V(final observation) is not negligible next to the reward
        shows = tr & (GAMMA * host(v_final) > 1e-3 * np.abs(host(p['rew'])))
        assert (host(col.adv)[shows] != host(plain_adv.t)[shows]).all(), iteration
        bootstrapped += int(shows.sum())
        assert (host(col.buf['trunc_t']) == np.where(tr.any(axis=0), tr.argmax(axis=0), -1)).all()
        assert tr.sum(axis=0).max() <= 1                                      # at most one truncation per env and collection
        truncated += int(tr.sum())
        live_slots += int(host(live).sum())
        # the episode log of the recorded slots
        log = col.episodes()
        want_log = collect.fold_episode_log(collect.episode_log_reference(host(col.buf['ret_buf']), host(col.buf['len_buf']), host(col.buf['code_buf'])))
        assert log['slots'] == Tn * B and log['episodes'] == int((host(p['code']) != 0).sum()) and log['nonfinite'] == 0
        for k, w in want_log.items():
            if k in ('return_mean', 'return_std', 'length_mean'):
                assert abs(log[k] - w) <= 1e-12 * max(abs(w), 1.0), (k, log[k], w)
            else:
                assert log[k] == w, (k, log[k], w)
        print('iteration %d: %d truncated (%d with a bootstrap that shows), %d live of %d slots; %s'
              % (iteration, int(tr.sum()), int(shows.sum()), int(host(live).sum()), Tn * B, log))
    assert truncated > 0 and live_slots > 0 and bootstrapped > 0              # otherwise the comparison proves nothing
    assert col.iteration == 2


def test_collector_refuses_what_it_cannot_run():
    from env_build_amd.endtoend import CrossroadEnd2end
    from tests import _epoch as E
    env = make_env()
    policy, value = E.make_nets()
    with pytest.raises(ValueError, match='max_episode_steps'):
        collect.Collector(env, policy, value, 6, 1.0)
    with pytest.raises(ValueError, match='auto_reset'):
        collect.Collector(CrossroadEnd2end('left', n_env=65, auto_reset=True, max_episode_steps=5), policy, value, 5, 1.0)
    with pytest.raises(TypeError):
        collect.Collector(object(), policy, value, 5, 1.0)
    with pytest.raises(ValueError, match='-> 1'):
        collect.Collector(env, policy, policy, 5, 1.0)
    policy.set_precision('fp16')
    with pytest.raises(ValueError, match='fp16'):
        collect.Collector(env, policy, value, 5, 1.0)
    policy.set_precision('fp32')
    assert collect.Collector(env, policy, value, 5, 1.0).steps == 5


# ---- 6: the example ---------------------------------------------------------------------------------------------------------------------------
def test_ppo_collect_loop_example_runs():
    spec = importlib.util.spec_from_file_location('ppo_collect_loop', os.path.join(ROOT, 'examples', 'ppo_collect_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.run(n_env=256, steps=8, iterations=2, epochs=2, minibatches=2, num_hidden_units=64, max_episode_steps=8)
    assert len(res['logs']) == 2 and len(res['episodes']) == 2
    for log in res['logs']:
        for name in ('policy_loss', 'value_loss', 'entropy', 'clip_fraction', 'approx_kl', 'max_ratio_dev'):
            assert log[name].shape == (2, 2) and np.isfinite(log[name]).all(), name
        assert (log['nonfinite_rows'] == 0).all() and (log['rows'] == 1024).all()
        assert log['max_ratio_dev'][0, 0] == 0.0 and log['approx_kl'][0, 0] == 0.0     # the replay read the refilled buffers: ratio exactly 1
    assert res['policy_delta'] > 0.0 and res['value_delta'] > 0.0
    assert res['optimiser_steps'] == 8 and res['counter'] == 4
    for ep in res['episodes']:
        assert ep['episodes'] > 0 and ep['slots'] == 2048 and ep['nonfinite'] == 0
        assert np.isfinite([ep['return_mean'], ep['return_std'], ep['length_mean'], ep['return_max'], ep['return_min']]).all()
    assert sum(ep['outcomes']['time_limit'] for ep in res['episodes']) > 0
