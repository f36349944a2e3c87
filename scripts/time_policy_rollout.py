#!/usr/bin/env python3
"""Profiling aid: the closed-loop rollout in one launch (eb_policy_rollout, csrc/eb_policy_rollout.hip) against the loop it replaces,
eb_shield_is_safe's two launches per look-ahead through the SAME fp16 handle, in ONE process on cuda:0, HIP events on the launch stream,
alternating windows, the discipline of scripts/time_policy_f16.py:

  (large)  65 536 envs x 32 vehicles, 137 -> 256 -> 256 -> 4, only punish / safe asked of the fused entry, at 5 and at 20 steps;
  (small)  4 096 envs x 8 vehicles, 41 -> 256 -> 256 -> 4, at 5 and at 20 steps — reported only.

The condition the large numbers are held to is printed as `holds_fused_faster_by_more_than_both_spreads`.  The two entries' flags and
sums are compared after the windows (`outputs_equal`).

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_rollout.py [--iters 20] [--windows 5] [--out FILE]"""
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
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15_policy_rollout_timing.txt'))
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


def alternate(fns):
    """-> {name: [us per pass, one per window]}: the entries take turns, window by window"""
    for fn in fns.values():
        for _ in range(3): fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.windows):
        for k, fn in fns.items():
            times[k].append(window(fn))
    return times


def case(what, n_env, n_veh, steps, hold):
    inp = make_rollout_inputs(a.task, n_env, n_veh, 1, seed=0)
    m = EnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(),
                                                   ego[:, 0].contiguous(), 0, ref_indexes=ref).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    D = obs0.shape[1]
    net = MLPNet(D, 2, 256, 'elu', 4, device=dev, precision='fp16')
    net.set_obs_scale(np.asarray([0.2] * 6 + [1., 1 / 30., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * n_veh, np.float32))
    ok = C.c_int32(0)
    m.api.policy_rollout_supported(m.handle, net._handle, C.byref(ok))
    assert ok.value == 1
    obs_a, obs_b, obs_f = torch.empty_like(obs0), torch.empty_like(obs0), torch.empty_like(obs0)
    actions = torch.empty((n_env, 2), dtype=torch.float32, device=dev); out5 = torch.empty((5, n_env), dtype=torch.float32, device=dev)
    punish = torch.empty((n_env,), dtype=torch.float32, device=dev); safe = torch.empty((n_env,), dtype=torch.uint8, device=dev)
    punish_f, safe_f = torch.empty_like(punish), torch.empty_like(safe)
    pen = _capi.PENALTY_ID['veh2veh4real' if steps == 5 else 'real_punish_term']
    fns = {'loop': lambda: m.api.shield_is_safe(m.handle, net._handle, n_env, p(obs0), p(ref), 0, steps, pen, C.c_float(1.0), p(obs_a),
                                                p(obs_b), p(actions), p(out5), p(punish), p(safe), _stream(dev)),
           'fused': lambda: m.api.policy_rollout(m.handle, net._handle, n_env, steps, p(obs0), p(ref), 0, C.c_float(1.0), pen, p(obs_f),
                                                 None, None, None, p(punish_f), p(safe_f), _stream(dev))}
    times = alternate(fns)
    us = {k: med(v) for k, v in times.items()}
    rec = dict(what=what, n_env=n_env, n_veh=n_veh, obs_dim=D, steps=steps, iters=a.iters, net='%d -> 256 -> 256 -> 4, elu / linear, fp16' % D)
    for k in times:
        rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(spread(times[k]))
    rec['loop_over_fused'] = round(us['loop'] / us['fused'], 2)
    rec['fused_us_per_step'] = r(us['fused'] / steps)
    if hold:
        rec['holds_fused_faster_by_more_than_both_spreads'] = bool(us['loop'] - us['fused'] > max(spread(times['loop']), spread(times['fused'])))
    for fn in fns.values(): fn()
    torch.cuda.synchronize()
    last = obs_a if steps % 2 == 1 else obs_b
    rec['outputs_equal'] = bool(torch.equal(safe, safe_f) and torch.equal(punish.view(torch.int32), punish_f.view(torch.int32))
                                and torch.equal(last.view(torch.int32), obs_f.view(torch.int32)))
    rec['safe_share'] = round(float(safe_f.float().mean()), 4)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


for steps in (5, 20):
    case('large', 65536, 32, steps, True)
for steps in (5, 20):
    case('small', 4096, 8, steps, False)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
