#!/usr/bin/env python3
"""Profiling aid: what the two device-side controls of the update phase cost — epochs x minibatches minibatches of `rows` rows out of
N = minibatches x rows, policy and value network obs_dim -> 256 -> 256 -> 4 | 1 — in ONE process on cuda:0, HIP events on the launch
stream, alternating windows, median with spread (the discipline of scripts/time_epoch.py and scripts/time_collect.py).  Two routes, each
on its own pair of networks made from the same weights, on the same data:

  (a) replay          epoch.PPOEpochs.replay() of one capture(): the parent's update phase
  (b) replay_ctl      ctl.PPOEpochs.replay() with a learning-rate table and a target_kl set — one eb_ctl_begin per iteration, one
                      eb_kl_stop (two launches) per minibatch, eb_adam_step_ctl in eb_adam_step's place.  The target is out of reach, so
                      every optimiser step is taken: the controlled route at its dearest (a stopped step returns early)

and the three new entries on their own, per call: (begin) eb_ctl_begin, (kl_stop) eb_kl_stop over one minibatch's rows, (adam_ctl)
eb_adam_step_ctl against (adam) eb_adam_step over the same two networks' segments, and (adam_ctl_stopped) eb_adam_step_ctl on a stopped
control block.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_ctl.py [--rows 4096] [--obs-dim 41] [--epochs 4] [--minibatches 4] [--iters 5] [--part-iters 100] [--windows 5]
                               [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import ctl, epoch, train
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=4096); ap.add_argument('--obs-dim', type=int, default=41)
ap.add_argument('--epochs', type=int, default=4); ap.add_argument('--minibatches', type=int, default=4)
ap.add_argument('--iters', type=int, default=5); ap.add_argument('--part-iters', type=int, default=100)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r27_ctl_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

rows, obs_dim, E, M = a.rows, a.obs_dim, a.epochs, a.minibatches
N = M * rows
clip, ent_coef, vf_coef, clip_v, lr, max_norm = 0.2, 1e-3, 0.5, 0.2, 1e-5, 0.5     # a small lr: hundreds of steps on one set of data
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
scale = rng.uniform(0.02, 0.2, obs_dim).astype(np.float32)


def nets():
    policy = TrainableMLPNet(obs_dim, 2, 256, 'elu', 4, output_activation='linear', device=dev, seed=0)
    value = TrainableMLPNet(obs_dim, 2, 256, 'elu', 1, output_activation='relu', device=dev, seed=1)
    policy.set_obs_scale(scale); value.set_obs_scale(scale)
    return policy, value


pol_a, val_a = nets(); pol_b, val_b = nets(); pol_p, val_p = nets()
obs = gpu(rng.standard_normal((N, obs_dim)) * 10)
actions = ps.sample_actions(pol_a, obs, 1.0, seed=1, want=())['actions'].t.clone()
logp_old = (pl.log_prob_actions(pol_a, obs, actions, 1.0)['logp'].t + gpu(rng.uniform(-0.4, 0.4, N))).contiguous()
adv = gpu(rng.standard_normal(N))
with torch.no_grad():
    v_old = val_a(obs)[:, 0].clone()
ret = v_old + gpu(rng.uniform(-0.6, 0.6, N))
data = dict(obs=obs, actions=actions.contiguous(), logp_old=logp_old, adv=adv, ret=ret, v_old=v_old)
kw = dict(ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_norm)
upd_a = train.PPOUpdate(pol_a, val_a, rows, 1.0, clip, **kw)
upd_b = ctl.PPOUpdate(pol_b, val_b, rows, 1.0, clip, lr_table=np.ones(8, np.float32), target_kl=1e9, max_slots=E * M, **kw)
loop_a = epoch.PPOEpochs(upd_a, data, E, M, seed=0)
loop_b = ctl.PPOEpochs(upd_b, data, E, M, seed=0)
graph_a, graph_b = loop_a.capture(), loop_b.capture()

# ---- the parts: one control block of their own, the segments of a third pair of networks ----
api, tapi = ctl.ctl_api(), train.train_api()
raw = pol_p._stream()
open_ctl = ctl.UpdateControl(dev, lr_table=np.ones(8, np.float32), target_kl=1e9, max_slots=4)
shut_ctl = ctl.UpdateControl(dev, max_slots=0)
open_ctl.begin()
shut_ctl.begin()
shut_ctl.buffer.view(torch.int32)[3] = 1                        # stopped
lp, lo = gpu(rng.standard_normal(rows)), gpu(rng.standard_normal(rows))
kl_args = open_ctl.kl_args(lp, lo, rows)
kl_args.stream = raw
plain = train.Adam([pol_p, val_p], lr=lr, max_grad_norm=max_norm)
for g in plain.grads:
    g.copy_(gpu(rng.standard_normal(g.numel()) * 1e-3))
plain._args.stream = raw
with_open = ctl.EbAdamCtlArgs(adam=plain._args, ctl=open_ctl.buffer.data_ptr())
with_shut = ctl.EbAdamCtlArgs(adam=plain._args, ctl=shut_ctl.buffer.data_ptr())
begin_args = open_ctl._begin
begin_args.stream = raw


def begin(): api.check(api.ctl_begin(C.byref(begin_args)))
def kl_stop(): api.check(api.kl_stop(C.byref(kl_args)))
def adam(): tapi.check(tapi.adam_step(C.byref(plain._args)))
def adam_ctl(): api.check(api.adam_step_ctl(C.byref(with_open)))
def adam_ctl_stopped(): api.check(api.adam_step_ctl(C.byref(with_shut)))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


routes = {'replay': lambda: loop_a.replay(graph_a), 'replay_ctl': lambda: loop_b.replay(graph_b)}
parts = {'begin': begin, 'kl_stop': kl_stop, 'adam': adam, 'adam_ctl': adam_ctl, 'adam_ctl_stopped': adam_ctl_stopped}
for fn in list(routes.values()) + list(parts.values()):
    for _ in range(2): fn()
torch.cuda.synchronize()
times = {k: [] for k in list(routes) + list(parts)}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn, a.iters))
    for k, fn in parts.items():
        times[k].append(window(fn, a.part_iters))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='ctl', rows=rows, N=N, epochs=E, minibatches=M, iters=a.iters, part_iters=a.part_iters,
           net='%d -> 256 -> 256 -> 4 | 1, elu / linear | relu, scale set, action_range 1' % obs_dim,
           adam_elements=int(sum(p.numel() for p in plain.params)),
           kernels={'replay': 3 + 15 * E * M, 'replay_ctl': 4 + 17 * E * M},
           unit='us per update phase (replay, replay_ctl) / per call (the parts)')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
rec['replay_ctl_minus_replay_us'] = r(us['replay_ctl'] - us['replay'])
rec['replay_ctl_over_replay'] = round(us['replay_ctl'] / us['replay'], 4)
rec['added_per_minibatch_us'] = r((us['replay_ctl'] - us['replay']) / (E * M))
rec['sum_of_parts_us'] = r(us['begin'] + E * M * (us['kl_stop'] + us['adam_ctl'] - us['adam']))
torch.cuda.synchronize()
log = loop_b.log()
rec['steps'] = {'replay': int(upd_a.adam.state.step), 'replay_ctl': int(upd_b.adam.state.step)}
rec['iterations_begun'] = upd_b.control.host()['iteration']
rec['applied_all'] = bool((log['applied'] == 1).all())
rec['same_weights'] = bool(all(torch.equal(x._flat, y._flat) for x, y in ((pol_a, pol_b), (val_a, val_b))))
rec['finite'] = bool(all(torch.isfinite(net._flat).all() for net in (pol_a, val_a, pol_b, val_b, pol_p, val_p)))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
