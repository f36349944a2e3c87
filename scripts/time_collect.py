#!/usr/bin/env python3
"""Profiling aid: the collection phase and the head of one PPO iteration — `steps` env steps of `n_env` envs, policy and value network
obs_dim -> 256 -> 256 -> 4 | 1 — in ONE process per shape on cuda:0, HIP events on the launch stream around the whole collection + head,
alternating windows, median with spread (the discipline of scripts/time_epoch.py).  Two routes, each on its own env (one seed) and its
own pair of networks made from the same weights:

  (a) parent      examples/ppo_epoch_loop.py's collection + head: four torch copies per step around sample_actions and env.step, two
                  value forwards, ppo.gae, log_prob_actions over all T * B rows
  (b) collector   Collector.collect() + Collector.finish()

and the parts on their own, per call, on synthetic buffers of the same shape: (record) eb_collect_record against (copies) the four torch
operations it replaces — three copy_ and copy_(code == 0); (head_parent) the parent's head against (head_collector) Collector.finish's
five launches.  --obs-dim other than the env's own width (41 for `left`) times the parts only: the env has no configuration of that
width under test, and the env step and eb_policy_sample are the same launches in both routes.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_collect.py [--n-env 4096] [--steps 32] [--obs-dim 41] [--iters 3] [--part-iters 50] [--windows 5] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import collect, ppo
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n-env', type=int, default=4096); ap.add_argument('--steps', type=int, default=32)
ap.add_argument('--obs-dim', type=int, default=41)
ap.add_argument('--iters', type=int, default=3); ap.add_argument('--part-iters', type=int, default=50)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r26_collect_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

B, T, D, GAMMA, LAM, SEED = a.n_env, a.steps, a.obs_dim, 0.99, 0.95, 0
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
scale = rng.uniform(0.02, 0.2, D).astype(np.float32)


def nets():
    policy = TrainableMLPNet(D, 2, 256, 'elu', 4, output_activation='linear', device=dev, seed=0)
    value = TrainableMLPNet(D, 2, 256, 'elu', 1, output_activation='relu', device=dev, seed=1)
    policy.set_obs_scale(scale); value.set_obs_scale(scale)
    return policy, value


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


routes, counts = {}, {}
with_env = D == 41
if with_env:
    from env_build_amd.endtoend import CrossroadEnd2end

    def make_env():
        env = CrossroadEnd2end('left', n_env=B, auto_reset=True, copy_outputs=False, max_episode_steps=max(T, 200))
        env.seed(SEED); env.reset(); env.reset()
        return env

    env_a, env_b = make_env(), make_env()
    pol_a, val_a = nets(); pol_b, val_b = nets()
    obs_buf = torch.empty((T, B, D), device=dev); act_buf = torch.empty((T, B, 2), device=dev)
    rew_buf = torch.empty((T, B), device=dev); live_buf = torch.empty((T, B), device=dev)
    counts['parent_iteration'] = 0

    def parent():
        it = counts['parent_iteration']; counts['parent_iteration'] += 1
        obs = env_a.obs
        for t in range(T):
            obs_buf[t].copy_(obs.t)
            out = ps.sample_actions(pol_a, obs_buf[t], 1.0, seed=SEED, counter=it * T + t, want=())
            act_buf[t].copy_(out['actions'].t)
            obs, reward, _done, _info = env_a.step(out['actions'])
            rew_buf[t].copy_(reward.t)
            live_buf[t].copy_(env_a.done_code == 0)
        obs_all, act_all = obs_buf.view(T * B, D), act_buf.view(T * B, 2)
        with torch.no_grad():
            v = val_a(obs_all)[:, 0].view(T, B).contiguous()
            v_last = val_a(obs.t)[:, 0].contiguous()
            adv, ret = ppo.gae(rew_buf, v, v_last, live_buf, GAMMA, LAM)
        return adv, ret, pl.log_prob_actions(pol_a, obs_all, act_all, 1.0)['logp'].t

    col = collect.Collector(env_b, pol_b, val_b, T, 1.0, seed=SEED)

    def collector():
        col.collect()
        return col.finish(GAMMA, LAM)

    routes = {'parent': parent, 'collector': collector}

# ---- the parts, on synthetic buffers ----
api = collect.collect_api()
pol_p, val_p = nets()
buf = collect.buffers(T, B, D, dev)
s_obs, s_final = gpu(rng.standard_normal((B, D))), gpu(rng.standard_normal((B, D)))
s_rew = gpu(rng.standard_normal(B))
s_code = torch.from_numpy((rng.integers(0, 8, B) * (rng.random(B) < 0.05)).astype(np.uint8)).to(dev)
p_obs = torch.empty((T, B, D), device=dev); p_act = gpu(rng.uniform(-0.9, 0.9, (T, B, 2)))
p_rew = torch.empty((T, B), device=dev); p_live = torch.empty((T, B), device=dev)
buf['obs_buf'].copy_(gpu(rng.standard_normal((T + 1, B, D)) * 10))
p_obs.copy_(buf['obs_buf'][:T])
logits = torch.empty((T, B, 4), device=dev)
rec_args = collect._record_args(T // 2, buf, s_obs, s_rew, s_code, s_final)
rec_args.stream = pol_p._stream()
values, v_trunc = torch.empty((T + 1, B), device=dev), torch.empty((B,), device=dev)
nv, logp_old = torch.empty((T, B), device=dev), torch.empty((T * B,), device=dev)
adv_o, ret_o = torch.empty((T, B), device=dev), torch.empty((T, B), device=dev)
nv_args = collect._next_values_args(values, v_trunc, buf['trunc_t'], nv)
lp_args = pl._args(None, T * B, 4, 1.0, logits=logits, actions=p_act, logp=logp_old)
gae_args = ppo._gae_args(None, T, B, GAMMA, LAM, rewards=buf['rew_buf'], values=values, nonterminal=buf['nonterminal'], next_values=nv,
                         carry=buf['carry'], adv=adv_o, ret=ret_o)
lp_fn, gae_fn = pl.bind(pol_p.api)['eb_policy_logp_from_logits'], ppo.bind(pol_p.api)['eb_gae']
for t in range(T):                                              # logits, rewards and flags a collection would have left
    pol_p.api.mlp_forward(pol_p._handle, B, C.c_void_p(p_obs[t].data_ptr()), C.c_void_p(logits[t].data_ptr()), pol_p._stream())
    a_t = collect._record_args(t, buf, s_obs, s_rew, s_code, s_final); a_t.stream = pol_p._stream()
    api.check(api.record(C.byref(a_t)))
p_rew.copy_(buf['rew_buf']); p_live.copy_(buf['carry'])


def record(): api.check(api.record(C.byref(rec_args)))


def copies():
    t = T // 2
    p_obs[t].copy_(s_obs); p_act[t].copy_(p_act[0]); p_rew[t].copy_(s_rew); p_live[t].copy_(s_code == 0)


def head_parent():
    obs_all, act_all = p_obs.view(T * B, D), p_act.view(T * B, 2)
    with torch.no_grad():
        v = val_p(obs_all)[:, 0].view(T, B).contiguous()
        v_last = val_p(s_obs)[:, 0].contiguous()
        out = ppo.gae(p_rew, v, v_last, p_live, GAMMA, LAM)
    return out, pl.log_prob_actions(pol_p, obs_all, act_all, 1.0)['logp'].t


def head_collector():
    s, h = pol_p._stream(), val_p._handle
    val_p.api.mlp_forward(h, (T + 1) * B, C.c_void_p(buf['obs_buf'].data_ptr()), C.c_void_p(values.data_ptr()), s)
    val_p.api.mlp_forward(h, B, C.c_void_p(buf['trunc_obs'].data_ptr()), C.c_void_p(v_trunc.data_ptr()), s)
    nv_args.stream = lp_args.stream = gae_args.stream = s
    api.check(api.next_values(C.byref(nv_args)))
    pol_p.api.check(lp_fn(C.byref(lp_args)))
    pol_p.api.check(gae_fn(C.byref(gae_args)))


parts = {'record': record, 'copies': copies}
heads = {'head_parent': head_parent, 'head_collector': head_collector}
for fn in list(routes.values()) + list(parts.values()) + list(heads.values()):
    for _ in range(2): fn()
torch.cuda.synchronize()
times = {k: [] for k in list(routes) + list(parts) + list(heads)}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn, a.iters))
    for k, fn in parts.items():
        times[k].append(window(fn, a.part_iters))
    for k, fn in heads.items():
        times[k].append(window(fn, a.iters))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='collect', n_env=B, steps=T, obs_dim=D, with_env=with_env, iters=a.iters, part_iters=a.part_iters,
           net='%d -> 256 -> 256 -> 4 | 1, elu / linear | relu, scale set, action_range 1' % D,
           record_bytes=2 * 4 * B * D + 4 * B * 8, unit='us per collection + head (parent, collector) / per call (the parts, the heads)')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
if with_env:
    rec['parent_over_collector'] = round(us['parent'] / us['collector'], 3)
    rec['per_step_us'] = {k: r((us[k] - us['head_' + k]) / T) for k in routes}
rec['copies_over_record'] = round(us['copies'] / us['record'], 3)
rec['record_GBps'] = r(rec['record_bytes'] / us['record'] / 1e3)
rec['head_parent_over_head_collector'] = round(us['head_parent'] / us['head_collector'], 3)
rec['steps_plus_head_saved_us'] = r(T * (us['copies'] - us['record']) + us['head_parent'] - us['head_collector'])
torch.cuda.synchronize()
rec['finite'] = bool(torch.isfinite(adv_o).all() and torch.isfinite(logp_old).all())
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
