#!/usr/bin/env python3
"""Profiling aid: cost and gradient of K candidate tapes per env (H = 25) three ways in ONE process on cuda:0 — HIP events on the
launch stream, alternating windows, the discipline of scripts/time_tape_cand.py:

  (new) one eb_rollout_tape_cand_vjp launch (csrc/eb_rollout_tape_cand_vjp.hip) with cost and g_action_tapes;
  (a)   K eb_rollout_tape_vjp launches from the same obs0: what a caller does today;
  (b)   one eb_rollout_tape_vjp launch over the rows replicated K times;
  (solver) one OpenLoopMPC.solve(starts='all') iteration over K starts against K single-start iterations, and one solve_paths
           iteration against 3 single-start iterations.

The ways are checked to give the same gradient bits before they are timed.  Every GPU step of a job that calls this runs under its
own `timeout`; results go to profiles/.

    python scripts/time_tape_cand_vjp.py [--shapes 65536x32,4096x16] [--cands 1,3,limit] [--iters 20] [--windows 5] [--solver-iterations 10]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd.cand import tape_cand_grad_max
from env_build_amd.dynamics_and_models import EnvironmentModel
from env_build_amd.mpc import OpenLoopMPC
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left'); ap.add_argument('--shapes', default='65536x32,4096x16', help='n_env x n_veh, comma separated')
ap.add_argument('--cands', default='1,3,limit'); ap.add_argument('--horizon', type=int, default=25); ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--windows', type=int, default=5); ap.add_argument('--solver-iterations', type=int, default=10)
a = ap.parse_args()
dev = torch.device('cuda', 0)
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
H = a.horizon
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
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
    vjp_fn, cg_fn = m.api.grad_fn('eb_rollout_tape_vjp'), m.api.cand_grad_fn('eb_rollout_tape_cand_vjp')
    w5 = (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0)
    ok = lambda rc: (_ for _ in ()).throw(RuntimeError(lib.eb_last_error())) if rc else None
    limit = tape_cand_grad_max(m, H)
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters): fn()
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    for K in sorted({limit if v == 'limit' else int(v) for v in a.cands.split(',') if v}):
        g = torch.Generator(device=dev).manual_seed(K)
        tapes = torch.stack([tape] + [(tape * (1.0 - 0.1 * k) + 0.2 * torch.randn(tape.shape, device=dev, generator=g)).clamp(-1, 1)
                                      for k in range(1, K)]).contiguous()
        out5 = torch.empty((K, H, 5, n_env), device=dev); cost = torch.empty((K, n_env), device=dev); gt = torch.empty_like(tapes)
        gk = torch.empty_like(tapes)
        obs_rep = obs0.repeat(K, 1).contiguous(); ref_rep = ref.repeat(K).contiguous()
        tape_rep = tapes.permute(1, 0, 2, 3).reshape(H, K * n_env, 2).contiguous()      # row k * n_env + e = candidate k of env e
        out5_rep = torch.empty((H, 5, K * n_env), device=dev); g_rep = torch.empty_like(tape_rep)
        def cand_vjp():
            ok(cg_fn(h, n_env, K, H, p(obs0), p(tapes), p(ref), 0, None, 0, 0, w5, p(out5), p(cost), None, p(gt), sp))
        def k_vjp():
            for k in range(K):
                ok(vjp_fn(h, n_env, H, p(obs0), p(tapes[k]), p(ref), 0, None, 0, None, w5, p(out5[k]), None, None, p(gk[k]), sp))
        def replicated_vjp():
            ok(vjp_fn(h, K * n_env, H, p(obs_rep), p(tape_rep), p(ref_rep), 0, None, 0, None, w5, p(out5_rep), None, None, p(g_rep), sp))
        fns = dict(cand_vjp=cand_vjp, k_vjp=k_vjp, replicated_vjp=replicated_vjp)
        for f in fns.values():
            for _ in range(3): f()
        torch.cuda.synchronize()
        # the three ways compute the same bits (the timing compares like with like)
        cand_vjp(); keep = out5.clone(); k_vjp(); replicated_vjp(); torch.cuda.synchronize()
        assert torch.equal(keep.view(torch.int32), out5.view(torch.int32)) and torch.equal(gt.view(torch.int32), gk.view(torch.int32))
        assert torch.equal(g_rep.view(H, K, n_env, 2).permute(1, 0, 2, 3).contiguous().view(torch.int32), gt.view(torch.int32))
        times = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, f in fns.items(): times[k].append(window(f))
        us = {k: med(v) for k, v in times.items()}
        r = lambda v: round(v, 1)
        print(json.dumps(dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, n_cand=K, limit=limit, iters=a.iters,
                              cand_vjp_us=r(us['cand_vjp']), cand_vjp_us_windows=[r(v) for v in times['cand_vjp']],
                              k_vjp_us=r(us['k_vjp']), k_vjp_us_windows=[r(v) for v in times['k_vjp']],
                              replicated_vjp_us=r(us['replicated_vjp']), replicated_vjp_us_windows=[r(v) for v in times['replicated_vjp']],
                              k_vjp_over_cand_vjp=round(us['k_vjp'] / us['cand_vjp'], 2),
                              replicated_over_cand_vjp=round(us['replicated_vjp'] / us['cand_vjp'], 2),
                              gain_over_k_vjp_us=r(us['k_vjp'] - us['cand_vjp']), k_vjp_spread_us=r(spread(times['k_vjp'])),
                              gain_over_replicated_us=r(us['replicated_vjp'] - us['cand_vjp']),
                              replicated_spread_us=r(spread(times['replicated_vjp'])))), flush=True)
        del tapes, out5, cost, gt, gk, obs_rep, ref_rep, tape_rep, out5_rep, g_rep, keep
    # one solver iteration: us per iteration from two solves of different length (the first evaluation and the allocations cancel),
    # in alternating windows
    mpc = OpenLoopMPC(m, horizon=H)
    k = a.solver_iterations
    K = min(3, limit)
    starts = torch.zeros((K, H, n_env, 2), device=dev)
    for s in range(1, K):
        starts[s, :, :, 1] = -1.0 if s == 1 else 1.0
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3
    ways = dict(
        all_starts=lambda it: mpc.solve(obs0, ref_indexes=ref, u_init=starts, starts='all', iterations=it),
        k_single_starts=lambda it: [mpc.solve(obs0, ref_indexes=ref, u_init=starts[s], iterations=it) for s in range(K)],
        solve_paths=lambda it: mpc.solve_paths(obs0, iterations=it),
        three_single_starts=lambda it: [mpc.solve(obs0, ref_indexes=torch.full_like(ref, q), iterations=it) for q in range(3)])
    if limit < 3:
        del ways['solve_paths'], ways['three_single_starts']
    for f in ways.values():
        f(k)                                                               # warm-up
    per_it = {n: [] for n in ways}
    for _ in range(a.windows):
        for name, f in ways.items():
            per_it[name].append((timed(lambda: f(2 * k)) - timed(lambda: f(k))) / k)
    out = dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, solver_iterations=k, n_starts=K)
    for name in ways:
        out['%s_us_per_iteration' % name] = round(med(per_it[name]), 1)
        out['%s_windows' % name] = [round(v, 1) for v in per_it[name]]
    out['k_single_over_all_starts'] = round(med(per_it['k_single_starts']) / med(per_it['all_starts']), 2)
    if 'solve_paths' in ways:
        out['three_single_over_solve_paths'] = round(med(per_it['three_single_starts']) / med(per_it['solve_paths']), 2)
    print(json.dumps(out), flush=True)
