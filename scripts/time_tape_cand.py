#!/usr/bin/env python3
"""Profiling aid: K candidate tapes per env (H = 25) scored three ways in ONE process on cuda:0 — HIP events on the launch stream,
alternating windows, the discipline of scripts/time_tape_vjp.py:

  (new) one eb_rollout_tape_cand launch (csrc/eb_rollout_tape_cand.hip) with out5_steps, and its cost-only form;
  (a)   K value-only eb_rollout_tape_vjp launches from the same obs0: what OpenLoopMPC's line search does by default;
  (b)   one eb_rollout_tape launch over the rows replicated K times: what a caller without the entry has to do;
  (solver) one OpenLoopMPC.solve iteration, fused_line_search against the default.

The ratio of the new launch at K = 3 and K = 8 to K = 1 is the direct test of the kernel's premise (the vehicles advance once per
env; the env role's wave fills with (env, candidate) lanes).  Every GPU step of a job that calls this runs under its own `timeout`;
results go to profiles/.

    python scripts/time_tape_cand.py [--shapes 65536x32,4096x16] [--cands 1,3,8] [--iters 20] [--windows 5] [--solver-iterations 10]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd.dynamics_and_models import EnvironmentModel
from env_build_amd.mpc import OpenLoopMPC
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left'); ap.add_argument('--shapes', default='65536x32,4096x16', help='n_env x n_veh, comma separated')
ap.add_argument('--cands', default='1,3,8'); ap.add_argument('--horizon', type=int, default=25); ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--windows', type=int, default=5); ap.add_argument('--solver-iterations', type=int, default=10)
ap.add_argument('--solvers', default='default,fused', help="which solvers to time (a kernel trace of one alone: --cands '' --solvers fused)")
a = ap.parse_args()
dev = torch.device('cuda', 0)
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
H = a.horizon
med = lambda v: sorted(v)[len(v) // 2]
for shape in a.shapes.split(','):
    n_env, n_veh = (int(v) for v in shape.split('x'))
    inp = make_rollout_inputs(a.task, n_env, n_veh, H, seed=0)
    m = EnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                                   0, ref_indexes=ref).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    tape = torch.from_numpy(inp['actions']).to(dev)
    st = torch.cuda.current_stream(); sp = C.c_void_p(st.cuda_stream)
    lib, h = m.api.lib, m.handle
    tape_fn, vjp_fn, cand_fn = lib.eb_rollout_tape, m.api.grad_fn('eb_rollout_tape_vjp'), m.api.cand_fn('eb_rollout_tape_cand')
    w5 = (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0)
    ok = lambda rc: (_ for _ in ()).throw(RuntimeError(lib.eb_last_error())) if rc else None
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters): fn()
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    new_us = {}
    for K in (int(v) for v in a.cands.split(',') if v):
        g = torch.Generator(device=dev).manual_seed(K)
        tapes = torch.stack([tape] + [(tape * (1.0 - 0.1 * k) + 0.2 * torch.randn(tape.shape, device=dev, generator=g)).clamp(-1, 1)
                                      for k in range(1, K)]).contiguous()
        out5 = torch.empty((K, H, 5, n_env), device=dev); cost = torch.empty((K, n_env), device=dev)
        obs_rep = obs0.repeat(K, 1).contiguous(); ref_rep = ref.repeat(K).contiguous()
        tape_rep = tapes.permute(1, 0, 2, 3).reshape(H, K * n_env, 2).contiguous()      # row k * n_env + e = candidate k of env e
        out5_rep = torch.empty((H, 5, K * n_env), device=dev); wk, fin = torch.empty_like(obs_rep), torch.empty_like(obs_rep)
        def cand_launch():
            ok(cand_fn(h, n_env, K, H, p(obs0), p(tapes), p(ref), 0, None, 0, 0, None, p(out5), None, sp))
        def cand_cost_only():
            ok(cand_fn(h, n_env, K, H, p(obs0), p(tapes), p(ref), 0, None, 0, 0, w5, None, p(cost), sp))
        def k_value_only():
            for k in range(K):
                ok(vjp_fn(h, n_env, H, p(obs0), p(tapes[k]), p(ref), 0, None, 0, None, w5, p(out5[k]), None, None, None, sp))
        def replicated_tape():
            ok(tape_fn(h, K * n_env, H, p(obs_rep), p(tape_rep), p(ref_rep), 0, p(wk), p(fin), p(out5_rep), sp))
        fns = dict(cand=cand_launch, cand_cost_only=cand_cost_only, k_value_only=k_value_only, replicated_tape=replicated_tape)
        for f in fns.values():
            for _ in range(3): f()
        torch.cuda.synchronize()
        # the three ways compute the same bits (the timing compares like with like)
        cand_launch(); keep = out5.clone(); k_value_only(); replicated_tape(); torch.cuda.synchronize()
        assert torch.equal(keep.view(torch.int32), out5.view(torch.int32))
        assert torch.equal(out5_rep.view(H, 5, K, n_env).permute(2, 0, 1, 3).contiguous().view(torch.int32), out5.view(torch.int32))
        times = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, f in fns.items(): times[k].append(window(f))
        us = {k: med(v) for k, v in times.items()}
        new_us[K] = us['cand']
        spread = lambda v: max(v) - min(v)
        print(json.dumps(dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, n_cand=K, iters=a.iters,
                              cand_us=round(us['cand'], 1), cand_us_windows=[round(v, 1) for v in times['cand']],
                              cand_cost_only_us=round(us['cand_cost_only'], 1),
                              k_value_only_us=round(us['k_value_only'], 1), k_value_only_us_windows=[round(v, 1) for v in times['k_value_only']],
                              replicated_tape_us=round(us['replicated_tape'], 1),
                              replicated_tape_us_windows=[round(v, 1) for v in times['replicated_tape']],
                              k_value_only_over_cand=round(us['k_value_only'] / us['cand'], 2),
                              replicated_tape_over_cand=round(us['replicated_tape'] / us['cand'], 2),
                              gain_over_k_value_only_us=round(us['k_value_only'] - us['cand'], 1), k_value_only_spread_us=round(spread(times['k_value_only']), 1),
                              gain_over_replicated_us=round(us['replicated_tape'] - us['cand'], 1), replicated_spread_us=round(spread(times['replicated_tape']), 1),
                              cand_over_cand_k1=round(us['cand'] / new_us[min(new_us)], 2) if min(new_us) == 1 else None)), flush=True)
        del tapes, out5, cost, obs_rep, ref_rep, tape_rep, out5_rep, wk, fin, keep
    # one solve iteration, fused against the default: us per iteration from two solves of different length (the first evaluation
    # and the allocations cancel), in alternating windows
    solvers = {n: OpenLoopMPC(m, horizon=H, fused_line_search=(n == 'fused')) for n in a.solvers.split(',') if n}
    def solve_us(mpc, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); _u, _J, info = mpc.solve(obs0, ref_indexes=ref, iterations=iters); e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, info
    k = a.solver_iterations
    per_it, lpi = {n: [] for n in solvers}, {}
    for mpc in solvers.values():
        solve_us(mpc, k)                                                   # warm-up
    for _ in range(a.windows):
        for name, mpc in solvers.items():
            t1, _ = solve_us(mpc, k); t2, info = solve_us(mpc, 2 * k)
            per_it[name].append((t2 - t1) / k); lpi[name] = info['launches_per_iteration']
    out = dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, solver_iterations=k)
    for name in solvers:
        out['%s_us_per_iteration' % name] = round(med(per_it[name]), 1)
        out['%s_windows' % name] = [round(v, 1) for v in per_it[name]]
        out['%s_launches_per_iteration' % name] = lpi[name]
    if len(solvers) == 2:
        out['default_over_fused'] = round(med(per_it['default']) / med(per_it['fused']), 2)
    print(json.dumps(out), flush=True)
