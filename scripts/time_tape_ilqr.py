#!/usr/bin/env python3
"""Profiling aid: one iLQR iteration (H = 25, 7 step lengths) against the first-order solver's building blocks, in ONE process on
cuda:0, HIP events on the launch stream, alternating windows, the discipline of scripts/time_tape_sample.py:

  (ilqr)       one eb_rollout_tape_ilqr launch (csrc/eb_rollout_tape_ilqr.hip) with gains from a previous launch: eight candidates per
               env scored, the best rolled out again, the model and the backward sweep;
  (ilqr_value) the same launch without gains_out: pass 1 and pass 2, no sweep (a solve's last launch);
  (ilqr_cost)  the same launch with cost / best_index / best_cost only: pass 1 alone;
               ilqr - ilqr_value and ilqr_value - ilqr_cost are what the sweep and pass 2 add;
  (tape_vjp)   one eb_rollout_tape_vjp launch, value and gradient;
  (pg_iter)    one iteration of the default solver (mpc.projected_gradient: ls_trials value-only launches, one gradient launch and
               its elementwise torch ops), timed as a one-iteration solve minus nothing: the start's gradient launch is included.

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_tape_ilqr.py [--shapes 4096x16,65536x32] [--iters 20] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd import ilqr
from env_build_amd.dynamics_and_models import EnvironmentModel
from env_build_amd.mpc import OpenLoopMPC, projected_gradient
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left')
ap.add_argument('--shapes', default='4096x16,65536x32', help='n_env x n_veh, comma separated')
ap.add_argument('--horizon', type=int, default=25); ap.add_argument('--iters', type=int, default=20); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12_tape_ilqr_timing.txt'))
a = ap.parse_args()
dev = torch.device('cuda', 0)
H = a.horizon
ALPHAS = (1, .5, .25, .125, .0625, .03125, .015625)
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
for shape in a.shapes.split(','):
    n_env, n_veh = (int(v) for v in shape.split('x'))
    inp = make_rollout_inputs(a.task, n_env, n_veh, H, seed=0)
    m = EnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                                   0, ref_indexes=ref).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    u0 = torch.from_numpy(inp['actions']).to(dev).clamp(-1, 1).contiguous()
    st = torch.cuda.current_stream()
    want = ('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv')
    first = ilqr.launch(m, obs0, u0, None, None, (), None, ref, 0, (-1.0, 10.0, 0.0, 0.0, 0.0), ilqr.alloc_outputs(H, n_env, 0, want, dev))
    out = ilqr.alloc_outputs(H, n_env, len(ALPHAS), want, dev)
    mu = torch.zeros(n_env, device=dev)
    al, w5 = (C.c_float * 7)(*ALPHAS), (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0)
    mpc = OpenLoopMPC(m, horizon=H)

    def t_ilqr():
        ilqr.launch(m, obs0, first['u'], first['x'], first['gains'], al, mu, ref, 0, w5, out)

    out_value = {k: v for k, v in out.items() if k not in ('gains', 'dv')}
    out_cost = {k: out[k] for k in ('cost', 'best_index', 'best_cost')}

    def t_ilqr_value():
        ilqr.launch(m, obs0, first['u'], first['x'], first['gains'], al, mu, ref, 0, w5, out_value)

    def t_ilqr_cost():
        ilqr.launch(m, obs0, first['u'], first['x'], first['gains'], al, mu, ref, 0, w5, out_cost)

    def t_vjp():
        mpc.value_and_grad(obs0, u0, ref, 0, need_grad=True)

    def t_pg():
        projected_gradient(lambda u, g: mpc.value_and_grad(obs0, u.contiguous(), ref, 0, g)[:2], u0, 1, ls_trials=mpc.ls_trials, c1=mpc.c1)
    fns = dict(ilqr=t_ilqr, ilqr_value=t_ilqr_value, ilqr_cost=t_ilqr_cost, tape_vjp=t_vjp, pg_iter=t_pg)
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    accepted = float((out['best_index'] > 0).float().mean())

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters): fn()
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    times = {k: [] for k in fns}
    for _ in range(a.windows):
        for k, fn in fns.items():
            times[k].append(window(fn))
    r = lambda v: round(v, 1)
    us = {k: med(v) for k, v in times.items()}
    rec = dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, n_alpha=len(ALPHAS), iters=a.iters, share_of_envs_that_accept_a_step=round(accepted, 3))
    for k in fns:
        rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(spread(times[k]))
    rec['pg_iter_includes'] = '1 start gradient launch + %d value-only launches + 1 gradient launch' % mpc.ls_trials
    rec['sweep_us'] = r(us['ilqr'] - us['ilqr_value']); rec['pass2_us'] = r(us['ilqr_value'] - us['ilqr_cost'])
    rec['ilqr_over_tape_vjp'] = round(us['ilqr'] / us['tape_vjp'], 2)
    rec['ilqr_over_pg_iter'] = round(us['ilqr'] / us['pg_iter'], 2)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)
    del m, mpc, out, first
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
