#!/usr/bin/env python3
"""Profiling aid: the running normalisation of observations and rewards (include/envbuild_norm.h) at one shape — `n_env` envs, `obs_dim`
floats — in ONE process on cuda:0, HIP events on the launch stream, alternating windows, median with spread (the discipline of
scripts/time_collect.py).  Per call, on synthetic buffers:

  (update)        eb_norm_update: the observation part and the return part together, two launches
  (apply)         eb_norm_apply: the next observation in place, the selected rows of trunc_obs and the reward, one launch
  (torch_update)  a torch twin of the same arithmetic: mean, var, merge (float64 state), the return recursion and its merge
  (torch_apply)   subtract, divide, clamp on the observations; divide, clamp on the rewards; the reset of the running return

and, at the env's own width (41 for `left`), the routes — each on its own env (one seed) and its own pair of networks of equal weights:

  (plain)         collect.Collector.collect() + finish(): the collection + head without normalisation
  (normalised)    norm.Collector.collect() + finish(): three more launches per env step

Timing is recorded, not asserted.  The rollout-buffer slot these calls work on fits the Infinity Cache, so the bytes per second below
are NOT HBM figures; at 4 096 envs every launch is launch-bound.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_norm.py [--n-env 4096] [--steps 32] [--obs-dim 41] [--iters 3] [--part-iters 100] [--windows 5] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import collect, norm
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n-env', type=int, default=4096); ap.add_argument('--steps', type=int, default=32)
ap.add_argument('--obs-dim', type=int, default=41)
ap.add_argument('--iters', type=int, default=3); ap.add_argument('--part-iters', type=int, default=100)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r29_norm_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

B, T, D, GAMMA, LAM, SEED, CLIP = a.n_env, a.steps, a.obs_dim, 0.99, 0.95, 0, 10.0
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


routes = {}
with_env = D == 41
if with_env:
    from env_build_amd.endtoend import CrossroadEnd2end

    def make_env():
        env = CrossroadEnd2end('left', n_env=B, auto_reset=True, copy_outputs=False, max_episode_steps=max(T, 200))
        env.seed(SEED); env.reset(); env.reset()
        return env

    def nets():
        return (TrainableMLPNet(D, 2, 256, 'elu', 4, output_activation='linear', device=dev, seed=0),
                TrainableMLPNet(D, 2, 256, 'elu', 1, output_activation='relu', device=dev, seed=1))

    col_a = collect.Collector(make_env(), *nets(), T, 1.0, seed=SEED)
    col_b = norm.Collector(make_env(), *nets(), T, 1.0, seed=SEED, gamma=GAMMA)

    def plain():
        col_a.collect()
        return col_a.finish(GAMMA, LAM)

    def normalised():
        col_b.collect()
        return col_b.finish(GAMMA, LAM)

    routes = {'plain': plain, 'normalised': normalised}

# ---- the parts, on synthetic buffers: one slot of a rollout buffer ----
api = norm.norm_api()
obs_state, ret_state = norm.NormState(D, dev), norm.NormState(1, dev)
slot = gpu(5.0 + 3.0 * rng.standard_normal((B, D)))
fresh = slot.clone()
trunc_obs, trunc_t = gpu(rng.standard_normal((B, D))), torch.from_numpy(np.where(rng.random(B) < 0.02, 3, -1).astype(np.int32)).to(dev)
reward, rew_slot, ret_run = gpu(-3.0 + 40.0 * rng.standard_normal(B)), torch.empty(B, device=dev), torch.zeros(B, device=dev)
code = torch.from_numpy((rng.integers(0, 8, B) * (rng.random(B) < 0.05)).astype(np.uint8)).to(dev)
u_args = norm._update_args(obs_state, slot, ret_state, reward, ret_run, GAMMA)
a_args = norm._apply_args(obs_state, slot, None, CLIP, trunc_obs, trunc_t, 3, ret_state, reward, rew_slot, code, ret_run, CLIP)[0]
u_args.stream = a_args.stream = st.cuda_stream
t_mean, t_var = torch.zeros(D, dtype=torch.float64, device=dev), torch.ones(D, dtype=torch.float64, device=dev)
t_ret = torch.zeros(B, device=dev); t_rmean = torch.zeros((), dtype=torch.float64, device=dev); t_rvar = torch.ones((), dtype=torch.float64, device=dev)
t_count = [1e-4, 1e-4]
t_out, t_rout = torch.empty_like(slot), torch.empty(B, device=dev)


def update(): api.check(api.update(C.byref(u_args)))


def apply():                                                      # (in place: the slot is re-normalised every call; the time does not depend on the values)
    api.check(api.apply(C.byref(a_args)))


def merge(mean, var, count, x):
    n = x.shape[0]
    bv, bm = torch.var_mean(x.double(), dim=0, unbiased=False)
    delta, tot = bm - mean, count + n
    M2 = var * count + bv * n + delta * delta * (count * n / tot)
    mean.add_(delta * (n / tot)); var.copy_(M2 / tot)
    return tot


def torch_update():
    t_count[0] = merge(t_mean, t_var, t_count[0], fresh)
    t_ret.mul_(GAMMA).add_(reward)
    t_count[1] = merge(t_rmean, t_rvar, t_count[1], t_ret)


def torch_apply():
    torch.clamp((fresh - t_mean.float()) / torch.sqrt(t_var.float() + 1e-8), -CLIP, CLIP, out=t_out)
    torch.clamp(reward / torch.sqrt(t_rvar.float() + 1e-8), -CLIP, CLIP, out=t_rout)
    t_ret.masked_fill_(code != 0, 0.0)


parts = {'update': update, 'apply': apply, 'torch_update': torch_update, 'torch_apply': torch_apply}
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
rec = dict(what='norm', n_env=B, steps=T, obs_dim=D, with_env=with_env, iters=a.iters, part_iters=a.part_iters,
           update_bytes=4 * B * D + 12 * B, apply_bytes=2 * 4 * B * D + 4 * B * 5 + B,
           unit='us per collection + head (plain, normalised) / per call (the parts)')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
if with_env:
    rec['normalised_over_plain'] = round(us['normalised'] / us['plain'], 3)
    rec['added_per_step_us'] = r((us['normalised'] - us['plain']) / T)
rec['torch_update_over_update'] = round(us['torch_update'] / us['update'], 3)
rec['torch_apply_over_apply'] = round(us['torch_apply'] / us['apply'], 3)
rec['update_GBps'] = r(rec['update_bytes'] / us['update'] / 1e3)
rec['apply_GBps'] = r(rec['apply_bytes'] / us['apply'] / 1e3)
torch.cuda.synchronize()
rec['finite'] = bool(torch.isfinite(obs_state.scale).all() and torch.isfinite(ret_state.scale).all() and torch.isfinite(slot).all())
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
