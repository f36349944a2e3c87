#!/usr/bin/env python3
"""Profiling aid: the closed-loop rollout with its parameter gradient in one call (csrc/eb_policy_rollout_grad.hip,
include/envbuild_policy_rollout_grad.h) against the composed path it replaces, in ONE process on cuda:0, HIP events on the launch
stream, alternating windows, the discipline of scripts/time_policy_grad.py.  25 steps each:

  (small)  1 024 envs x 8 slots, 41 -> 64 -> 64 -> 4;
  (mid)    4 096 envs x 8 slots, 41 -> 256 -> 256 -> 4;
  (large)  65 536 envs x 32 slots, 137 -> 256 -> 256 -> 4 — reported only, fewer calls per window, no autograd side.

Sides: `fused` (eb_policy_rollout_grad with cost and g_params), `fused_no_g_params` (the first launch alone: the difference is the
row reduction's two launches), `c_loop` (the loop of eb_policy_run_batch / eb_rollout_step / eb_rollout_step_vjp / eb_mlp_backward with
every buffer and the workspace allocated once, the per-step g_params added up), `autograd` (examples/adp_policy_gradient.py's
rollout_loss(...).backward() through torch).  The bar of (small) and (mid): `fused` under `c_loop` by more than the larger window
spread; `bar_met` says so.

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_rollout_grad.py [--iters 10] [--windows 5] [--skip-large] [--out FILE]"""
import argparse, ctypes as C, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.grad import DifferentiableEnvironmentModel
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=10); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--skip-large', action='store_true')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r17_policy_rollout_grad_timing.txt'))
a = ap.parse_args()
spec = importlib.util.spec_from_file_location('adp_policy_gradient', os.path.join(ROOT, 'examples', 'adp_policy_gradient.py'))
adp = importlib.util.module_from_spec(spec); spec.loader.exec_module(adp)
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
r = lambda v: round(v, 1)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
STEPS, LAM = 25, 10.0


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, iters):
    """{name: fn} -> {name: [us per call, one per window]}, the sides taking turns window by window"""
    for fn in fns.values():
        for _ in range(2): fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.windows):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def case(what, n, n_veh, units, iters, autograd=True, bar=True):
    model = DifferentiableEnvironmentModel('left', mode='training', n_veh=n_veh)
    D, api, h = model.obs_dim, model.api, model.handle
    obs0, ref = adp.start_states(model, n, 0)
    ri = ref.to(torch.int32).contiguous()
    net = TrainableMLPNet(D, 2, units, 'elu', 4, device=dev)
    rng = np.random.default_rng(0)
    net.set_obs_scale(rng.uniform(0.02, 0.2, D).astype(np.float32))
    net._sync()
    m, s = net._h, _stream(dev)
    w5v = [-1.0 / (STEPS * n), LAM / (STEPS * n), 0.0, 0.0, 0.0]
    w5 = (C.c_float * 5)(*w5v)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    # fused
    need = C.c_size_t(0)
    api.policy_rollout_grad_workspace_bytes(h, m, n, STEPS, C.byref(need))
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    cost, g_par = f32(n), torch.empty_like(net._flat)
    fused = lambda: api.policy_rollout_grad(h, m, n, STEPS, p(obs0), p(ri), 0, C.c_float(1.0), w5, p(ws), need.value, None, None, None, None,
                                            p(cost), None, None, p(g_par), s)
    first = lambda: api.policy_rollout_grad(h, m, n, STEPS, p(obs0), p(ri), 0, C.c_float(1.0), w5, p(ws), need.value, None, None, None, None,
                                            p(cost), None, None, None, s)
    # the loop of C calls, everything allocated once
    need1 = C.c_size_t(0)
    api.mlp_backward_workspace_bytes(m, n, C.byref(need1))
    ws1 = torch.empty((need1.value,), dtype=torch.uint8, device=dev)
    pre, acts, out5, scaled = f32(STEPS + 1, n, D), f32(STEPS, n, 2), f32(STEPS, 5, n), f32(n, 2)
    pre[0] = obs0
    g5 = torch.tensor(w5v, dtype=torch.float32, device=dev).view(5, 1).expand(5, n).contiguous()
    lam, sgo, pt, g_act = [f32(n, 9), f32(n, 9)], f32(n, 9), f32(n, D), f32(STEPS, n, 2)
    g_step, g_sum = torch.empty_like(net._flat), torch.empty_like(net._flat)
    vjp = api.grad_fn('eb_rollout_step_vjp')

    def c_loop():
        for t in range(STEPS):
            api.policy_run_batch(m, n, p(pre[t]), C.c_float(1.0), p(acts[t]), s)
            api.rollout_step(h, n, p(pre[t]), p(acts[t]), p(ri), 0, p(pre[t + 1]), p(out5[t]), p(scaled), s)
        lam[0].zero_(); g_sum.zero_()
        for k, t in enumerate(range(STEPS - 1, -1, -1)):
            a_, b_ = lam[k & 1], lam[1 - (k & 1)]
            vjp(h, n, p(pre[t]), p(acts[t]), p(ri), 0, p(a_), 9, p(g5), p(sgo), 9, p(g_act[t]), s)
            api.mlp_backward(m, n, p(pre[t]), p(g_act[t]), 1, C.c_float(1.0), p(ws1), need1.value, None, p(pt), p(g_step), s)
            torch.add(sgo, pt[:, :9], out=b_)
            g_sum.add_(g_step)

    fns = {'fused': fused, 'fused_no_g_params': first, 'c_loop': c_loop}
    if autograd:
        def through_torch():
            for q in net.parameters():
                q.grad = None
            adp.rollout_loss(model, lambda o: net.mode(o, 1.0), obs0, ref, STEPS, LAM).backward()
        fns['autograd'] = through_torch
    fused(); c_loop(); torch.cuda.synchronize()
    rel = float((g_par - g_sum).abs().max() / g_sum.abs().max())
    times = alternate(fns, iters)
    rec = dict(what=what, iters=iters, n=n, n_veh=n_veh, steps=STEPS, net='%d -> %d -> %d -> 4, elu / linear, scale set' % (D, units, units),
               workspace_mb=r(need.value / 2 ** 20), g_params_max_rel_diff_from_c_loop=rel)
    for k, v in times.items():
        rec[k + '_us'] = r(med(v)); rec[k + '_us_windows'] = [r(x) for x in v]; rec[k + '_spread_us'] = r(spread(v))
    rec['row_reduction_us'] = r(med(times['fused']) - med(times['fused_no_g_params']))
    if bar:
        rec['bar_met'] = bool(med(times['c_loop']) - med(times['fused']) > max(spread(times['c_loop']), spread(times['fused'])))
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


case('small', 1024, 8, 64, a.iters)
case('mid', 4096, 8, 256, a.iters)
if not a.skip_large:
    case('large', 65536, 32, 256, max(1, a.iters // 5), autograd=False, bar=False)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
