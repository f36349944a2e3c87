#!/usr/bin/env python3
"""Profiling aid: the policy network in fp32 (csrc/eb_policy.hip) against the opt-in fp16 kernel (csrc/eb_policy_f16.hip), in ONE process
on cuda:0, HIP events on the launch stream, alternating windows, the discipline of scripts/time_tape_ilqr.py:

  (policy)  eb_policy_run_batch at 65 536 x (137 -> 256 -> 256 -> 4), elu hidden, linear out, scale set, action_range 1;
  (small)   the same at 4 096 x (41 -> 256 -> 256 -> 4);
  (shield)  eb_shield_is_safe, 5 look-aheads at 65 536 envs x 32 vehicles (policy launch + rollout launch per look-ahead).

Both precisions run through ONE handle switched with eb_mlp_set_precision between windows, so the weights, buffers and launch path
are the same.  The conditions the numbers are held to are printed as `holds_*` (fp16 at most half the fp32 launch and clear of it by
more than either spread; the fp16 shield faster by more than both spreads).

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_f16.py [--iters 20] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import _capi
from env_build_amd.dynamics_and_models import EnvironmentModel, _stream
from env_build_amd.policy import MLPNet
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left')
ap.add_argument('--iters', type=int, default=20); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r14_policy_f16_timing.txt'))
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
r = lambda v: round(v, 1)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


def alternate(net, fn):
    """-> {'fp32': [us per call, one per window], 'fp16': [...]}: the handle switched between windows"""
    for prec in ('fp32', 'fp16'):
        net.set_precision(prec)
        for _ in range(3): fn()
    torch.cuda.synchronize()
    times = {'fp32': [], 'fp16': []}
    for _ in range(a.windows):
        for prec in times:
            net.set_precision(prec)
            times[prec].append(window(fn))
    return times


def record(what, times, **extra):
    us = {k: med(v) for k, v in times.items()}
    rec = dict(what=what, iters=a.iters, **extra)
    for k in times:
        rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(spread(times[k]))
    rec['fp32_over_fp16'] = round(us['fp32'] / us['fp16'], 2)
    rec['holds_faster_by_more_than_both_spreads'] = bool(us['fp32'] - us['fp16'] > max(spread(times['fp32']), spread(times['fp16'])))
    return rec, us


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def policy_case(what, n, obs_dim):
    rng = np.random.default_rng(0)
    net = MLPNet(obs_dim, 2, 256, 'elu', 4, device=dev)
    net.set_obs_scale(rng.uniform(0.02, 0.2, obs_dim).astype(np.float32))
    obs = torch.from_numpy((rng.standard_normal((n, obs_dim)) * 10).astype(np.float32)).to(dev)
    out = torch.empty((n, 2), dtype=torch.float32, device=dev)
    fn = lambda: net.api.policy_run_batch(net._handle, n, p(obs), C.c_float(1.0), p(out), _stream(dev))
    rec, us = record(what, alternate(net, fn), n=n, net='%d -> 256 -> 256 -> 4, elu / linear, scale set, action_range 1' % obs_dim)
    return rec, us


rec, us = policy_case('policy', 65536, 137)
rec['holds_fp16_at_most_half_of_fp32'] = bool(us['fp16'] <= 0.5 * us['fp32'])
emit(rec)
rec, us = policy_case('small', 4096, 41)
emit(rec)

n_env, n_veh, steps = 65536, 32, 5
inp = make_rollout_inputs(a.task, n_env, n_veh, 1, seed=0)
m = EnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                               0, ref_indexes=ref).t
obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
D = obs0.shape[1]
net = MLPNet(D, 2, 256, 'elu', 4, device=dev)
net.set_obs_scale(np.asarray([0.2] * 6 + [1., 1 / 30., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * n_veh, np.float32))
obs_a, obs_b = torch.empty_like(obs0), torch.empty_like(obs0)
actions = torch.empty((n_env, 2), dtype=torch.float32, device=dev); out5 = torch.empty((5, n_env), dtype=torch.float32, device=dev)
punish = torch.empty((n_env,), dtype=torch.float32, device=dev); safe = torch.empty((n_env,), dtype=torch.uint8, device=dev)
fn = lambda: m.api.shield_is_safe(m.handle, net._handle, n_env, p(obs0), p(ref), 0, steps, _capi.PENALTY_ID['veh2veh4real'], C.c_float(1.0),
                                  p(obs_a), p(obs_b), p(actions), p(out5), p(punish), p(safe), _stream(dev))
times = alternate(net, fn)
flags = {}
for prec in ('fp32', 'fp16'):
    net.set_precision(prec); fn(); torch.cuda.synchronize()
    flags[prec] = safe.clone()
rec, us = record('shield', times, n_env=n_env, n_veh=n_veh, look_aheads=steps, obs_dim=D)
for k in ('fp32', 'fp16'):
    rec[k + '_checks_per_s'] = round(n_env / (us[k] * 1e-6))
rec['safe_share_fp32'] = round(float(flags['fp32'].float().mean()), 4)
rec['flags_that_differ'] = int((flags['fp32'] != flags['fp16']).sum())
emit(rec)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
