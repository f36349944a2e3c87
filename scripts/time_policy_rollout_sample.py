#!/usr/bin/env python3
"""Profiling aid: the stochastic closed-loop rollout with its reparameterised parameter gradient in one call
(csrc/eb_policy_rollout_sample.hip, include/envbuild_policy_rollout_sample.h) against the composed path it replaces, in ONE process on
cuda:0, HIP events on the launch stream, alternating windows, the discipline of scripts/time_policy_rollout_grad.py.  25 steps each;
cost, logp_steps and g_params asked for:

  (small)  1 024 envs x 8 slots, 41 -> 64 -> 64 -> 4;
  (mid)    4 096 envs x 8 slots, 41 -> 256 -> 256 -> 4;
  (large)  65 536 envs x 32 slots, 137 -> 256 -> 256 -> 4 — reported only, fewer calls per window.

Sides: `fused` (eb_policy_rollout_sample with cost, logp_steps and g_params: three launches), `fused_forward_only` (cost and logp_steps,
no gradient pointer: one launch, no workspace), `c_loop` (the loop of eb_policy_sample / eb_rollout_step forward and eb_rollout_step_vjp
/ eb_policy_sample_vjp / eb_mlp_backward back with every buffer and the workspace allocated once, the per-step g_params added up),
`deterministic` (eb_policy_rollout_grad with cost and g_params: what the sampling head costs on top of the parent kernel).  The bar of
(small) and (mid) is that script's: `fused` under `c_loop` by more than the larger window spread; `bar_met` says so.

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_rollout_sample.py [--iters 10] [--windows 5] [--skip-large] [--out FILE]"""
import argparse, ctypes as C, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.grad import DifferentiableEnvironmentModel
from env_build_amd import policy_rollout as PR, policy_sample as PS
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=10); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--skip-large', action='store_true')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_policy_rollout_sample_timing.txt'))
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
STEPS, LAM, ALPHA, SEED = 25, 10.0, 0.05, 7


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


def case(what, n, n_veh, units, iters, bar=True):
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
    w_logp = ALPHA / (STEPS * n)
    w5 = (C.c_float * 5)(*w5v)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    raw = lambda t: t.data_ptr()
    fn, sample = PR.bind_sample(api), PS.bind(api)
    # fused
    need = C.c_size_t(0)
    api.check(fn['eb_policy_rollout_sample_workspace_bytes'](h, m, n, STEPS, 1, C.byref(need)))
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    cost, logp, g_par = f32(n), f32(STEPS, n), torch.empty_like(net._flat)
    common = dict(n_env=n, steps=STEPS, action_range=1.0, w_logp=w_logp, w5=w5v, seed=SEED, counter=0, obs_in=raw(obs0), ref_idx=raw(ri),
                  cost=raw(cost), logp_steps=raw(logp), stream=s)
    a_full = PR.sample_args(workspace=raw(ws), workspace_bytes=need.value, g_params=raw(g_par), **common)
    a_fwd = PR.sample_args(**common)
    run = fn['eb_policy_rollout_sample']
    fused = lambda: api.check(run(h, m, C.byref(a_full)))
    forward = lambda: api.check(run(h, m, C.byref(a_fwd)))
    # the deterministic parent
    need0 = C.c_size_t(0)
    api.policy_rollout_grad_workspace_bytes(h, m, n, STEPS, C.byref(need0))
    ws0 = torch.empty((need0.value,), dtype=torch.uint8, device=dev)
    cost0, g_par0 = f32(n), torch.empty_like(net._flat)
    parent = lambda: api.policy_rollout_grad(h, m, n, STEPS, p(obs0), p(ri), 0, C.c_float(1.0), w5, p(ws0), need0.value, None, None, None, None,
                                             p(cost0), None, None, p(g_par0), s)
    # the loop of C calls, everything allocated once
    need1 = C.c_size_t(0)
    api.mlp_backward_workspace_bytes(m, n, C.byref(need1))
    ws1 = torch.empty((need1.value,), dtype=torch.uint8, device=dev)
    pre, acts, out5, scaled = f32(STEPS + 1, n, D), f32(STEPS, n, 2), f32(STEPS, 5, n), f32(n, 2)
    lps, ys, used, g_y = f32(STEPS, n), f32(STEPS, n, 4), f32(STEPS, n, 2), f32(n, 4)
    pre[0] = obs0
    g5 = torch.tensor(w5v, dtype=torch.float32, device=dev).view(5, 1).expand(5, n).contiguous()
    g_lp = torch.full((n,), w_logp, dtype=torch.float32, device=dev)
    lam, sgo, pt, g_act = [f32(n, 9), f32(n, 9)], f32(n, 9), f32(n, D), f32(STEPS, n, 2)
    g_step, g_sum = torch.empty_like(net._flat), torch.empty_like(net._flat)
    vjp = api.grad_fn('eb_rollout_step_vjp')
    one, back = sample['eb_policy_sample'], sample['eb_policy_sample_vjp']

    def c_loop():
        for t in range(STEPS):
            one(m, n, raw(pre[t]), None, None, SEED, t, 1.0, raw(acts[t]), raw(lps[t]), raw(ys[t]), raw(used[t]), s)
            api.rollout_step(h, n, p(pre[t]), p(acts[t]), p(ri), 0, p(pre[t + 1]), p(out5[t]), p(scaled), s)
        lam[0].zero_(); g_sum.zero_()
        for k, t in enumerate(range(STEPS - 1, -1, -1)):
            a_, b_ = lam[k & 1], lam[1 - (k & 1)]
            vjp(h, n, p(pre[t]), p(acts[t]), p(ri), 0, p(a_), 9, p(g5), p(sgo), 9, p(g_act[t]), s)
            back(n, 4, raw(ys[t]), raw(used[t]), 1.0, raw(g_act[t]), raw(g_lp), raw(g_y), s)
            api.mlp_backward(m, n, p(pre[t]), p(g_y), 0, C.c_float(0.0), p(ws1), need1.value, None, p(pt), p(g_step), s)
            torch.add(sgo, pt[:, :9], out=b_)
            g_sum.add_(g_step)

    fns = {'fused': fused, 'fused_forward_only': forward, 'c_loop': c_loop, 'deterministic': parent}
    fused(); c_loop(); torch.cuda.synchronize()
    rel = float((g_par - g_sum).abs().max() / g_sum.abs().max())
    same_logp = bool(torch.equal(logp, lps))
    times = alternate(fns, iters)
    rec = dict(what=what, iters=iters, n=n, n_veh=n_veh, steps=STEPS, net='%d -> %d -> %d -> 4, elu / linear, scale set' % (D, units, units),
               workspace_mb=r(need.value / 2 ** 20), g_params_max_rel_diff_from_c_loop=rel, logp_equals_c_loop=same_logp)
    for k, v in times.items():
        rec[k + '_us'] = r(med(v)); rec[k + '_us_windows'] = [r(x) for x in v]; rec[k + '_spread_us'] = r(spread(v))
    rec['head_over_deterministic_us'] = r(med(times['fused']) - med(times['deterministic']))
    if bar:
        rec['bar_met'] = bool(med(times['c_loop']) - med(times['fused']) > max(spread(times['c_loop']), spread(times['fused'])))
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


case('small', 1024, 8, 64, a.iters)
case('mid', 4096, 8, 256, a.iters)
if not a.skip_large:
    case('large', 65536, 32, 256, max(1, a.iters // 5), bar=False)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
