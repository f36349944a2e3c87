#!/usr/bin/env python3
"""Profiling aid: the update phase of one PPO iteration — epochs x minibatches minibatches of `rows` rows out of N = minibatches x rows,
policy and value network obs_dim -> 256 -> 256 -> 4 | 1 — in ONE process on cuda:0, HIP events on the launch stream, alternating windows
(the discipline of scripts/time_train.py).  Three routes, each on its own pair of networks made from the same weights:

  (a) parent          examples/ppo_captured_loop.py's update phase: adv.mean() / adv.std() through torch, torch.randperm per epoch, six
                      torch.index_select(..., out=) and one PPOUpdate.replay() per minibatch, the logging expressions with their
                      float() host reads once per epoch
  (b) step            PPOEpochs.step(), eager
  (c) replay          PPOEpochs.replay() of one PPOEpochs.capture()

and the parts on their own, per call: (gather) eb_minibatch_gather of one minibatch under the keyed shuffle, (gather_perm) the same with
an explicit int64 permutation, (index_select) the six torch.index_select(..., out=) launches it replaces, (copy) six copy_ of the same
rows in order — the bytes of the gather without an index —, (randperm) torch.randperm(N), (stats) eb_adv_stats against (stats_torch)
torch.stack([adv.mean(), 1 / (adv.std() + 1e-8)]), (log) eb_ppo_log against (log_torch) the example's five logging expressions with
their host reads.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_epoch.py [--rows 65536] [--obs-dim 137] [--epochs 4] [--minibatches 4] [--iters 5] [--part-iters 100]
                                 [--windows 5] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import epoch, train
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=65536); ap.add_argument('--obs-dim', type=int, default=137)
ap.add_argument('--epochs', type=int, default=4); ap.add_argument('--minibatches', type=int, default=4)
ap.add_argument('--iters', type=int, default=5); ap.add_argument('--part-iters', type=int, default=100)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r25_epoch_timing.txt'))
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


pol_a, val_a = nets(); pol_b, val_b = nets(); pol_c, val_c = nets()
obs = gpu(rng.standard_normal((N, obs_dim)) * 10)
actions = ps.sample_actions(pol_a, obs, 1.0, seed=1, want=())['actions'].t.clone()
logp_old = (pl.log_prob_actions(pol_a, obs, actions, 1.0)['logp'].t + gpu(rng.uniform(-0.4, 0.4, N))).contiguous()
adv = gpu(rng.standard_normal(N))
with torch.no_grad():
    v_old = val_a(obs)[:, 0].clone()
ret = v_old + gpu(rng.uniform(-0.6, 0.6, N))
data = dict(obs=obs, actions=actions.contiguous(), logp_old=logp_old, adv=adv, ret=ret, v_old=v_old)
FIELDS = ('obs', 'actions', 'logp_old', 'adv', 'ret', 'v_old')
kw = dict(ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_norm)
upd_a = train.PPOUpdate(pol_a, val_a, rows, 1.0, clip, **kw)
upd_b = train.PPOUpdate(pol_b, val_b, rows, 1.0, clip, **kw)
upd_c = train.PPOUpdate(pol_c, val_c, rows, 1.0, clip, **kw)
graph_a = upd_a.capture()
loop_b = epoch.PPOEpochs(upd_b, data, E, M, seed=0)
loop_c = epoch.PPOEpochs(upd_c, data, E, M, seed=0)
graph_c = loop_c.capture()
last = {}


def parent():
    adv_norm = torch.stack([adv.mean(), 1.0 / (adv.std() + 1e-8)])
    upd_a.mb.adv_norm.copy_(adv_norm)
    for _e in range(E):
        perm = torch.randperm(N, device=dev)
        for k in range(M):
            idx = perm[k * rows:(k + 1) * rows]
            for name in FIELDS:
                torch.index_select(data[name], 0, idx, out=getattr(upd_a.mb, name))
            upd_a.replay(graph_a)
        q = upd_a.rows
        last.update(policy_loss=float(-q.surr.mean()), value_loss=float(q.vloss.mean()), entropy=float(q.ent.mean()),
                    clip_fraction=float(((q.ratio - 1.0).abs() > clip).float().mean()), approx_kl=float((upd_a.mb.logp_old - q.logp).mean()))


# ---- the parts ----
api = epoch.epoch_api()
mb = upd_b.mb
dests = [getattr(mb, name) for name in FIELDS]
srcs = [data[name] for name in FIELDS]
perm64 = torch.randperm(N, device=dev)
g_keyed = epoch._gather_args(srcs, dests, rows, rows, None, 0, 1, loop_b.counter, None)
g_perm = epoch._gather_args(srcs, dests, rows, rows, perm64, 0, 0, None, None)
g_keyed.stream = g_perm.stream = upd_b.policy._stream()
idx = perm64[rows:2 * rows]
norm_out = torch.empty((2,), device=dev)
partials = torch.zeros((2 * epoch.EB_EPOCH_PARTIALS,), dtype=torch.float64, device=dev)
s_args = epoch.EbAdvStatsArgs(n=N, x=adv.data_ptr(), eps=1e-8, out=norm_out.data_ptr(), partials=partials.data_ptr(), stream=g_keyed.stream)
log_out = torch.zeros((epoch.EB_EPOCH_LOG_BLOCKS, epoch.EB_EPOCH_LOG_FIELDS), dtype=torch.float64, device=dev)
l_args = epoch._log_args(upd_b.rows, mb.logp_old, clip, log_out)
l_args.stream = g_keyed.stream


def gather(): api.check(api.minibatch_gather(C.byref(g_keyed)))
def gather_perm(): api.check(api.minibatch_gather(C.byref(g_perm)))
def stats(): api.check(api.adv_stats(C.byref(s_args)))
def log(): api.check(api.ppo_log(C.byref(l_args)))
def randperm(): return torch.randperm(N, device=dev)
def stats_torch(): return torch.stack([adv.mean(), 1.0 / (adv.std() + 1e-8)])


def index_select():
    for name, dst in zip(FIELDS, dests):
        torch.index_select(data[name], 0, idx, out=dst)


def copy():
    for name, dst in zip(FIELDS, dests):
        dst.copy_(data[name][rows:2 * rows])


def log_torch():
    q = upd_b.rows
    return (float(-q.surr.mean()), float(q.vloss.mean()), float(q.ent.mean()), float(((q.ratio - 1.0).abs() > clip).float().mean()),
            float((mb.logp_old - q.logp).mean()))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


routes = {'parent': parent, 'step': loop_b.step, 'replay': lambda: loop_c.replay(graph_c)}
parts = {'gather': gather, 'gather_perm': gather_perm, 'index_select': index_select, 'copy': copy, 'randperm': randperm, 'stats': stats,
         'stats_torch': stats_torch, 'log': log, 'log_torch': log_torch}
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
row_bytes = 4 * (obs_dim + actions.shape[1] + 4)
rec = dict(what='epoch', rows=rows, N=N, epochs=E, minibatches=M, iters=a.iters, part_iters=a.part_iters,
           net='%d -> 256 -> 256 -> 4 | 1, elu / linear | relu, scale set, action_range 1' % obs_dim,
           gather_bytes=2 * rows * row_bytes, unit='us per update phase (parent, step, replay) / per call (the parts)')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
rec['parent_over_step'] = round(us['parent'] / us['step'], 3)
rec['parent_over_replay'] = round(us['parent'] / us['replay'], 3)
rec['per_minibatch_us'] = {k: r(us[k] / (E * M)) for k in routes}
rec['index_select_over_gather'] = round(us['index_select'] / us['gather'], 3)
rec['gather_over_copy'] = round(us['gather'] / us['copy'], 3)
rec['gather_GBps'] = r(rec['gather_bytes'] / us['gather'] / 1e3)
rec['copy_GBps'] = r(rec['gather_bytes'] / us['copy'] / 1e3)
rec['stats_torch_over_stats'] = round(us['stats_torch'] / us['stats'], 3)
rec['log_torch_over_log'] = round(us['log_torch'] / us['log'], 3)
torch.cuda.synchronize()
rec['steps'] = {k: int(u.adam.state.step) for k, u in (('parent', upd_a), ('step', upd_b), ('replay', upd_c))}
rec['finite'] = bool(all(torch.isfinite(net._flat).all() for net in (pol_a, val_a, pol_b, val_b, pol_c, val_c)))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
