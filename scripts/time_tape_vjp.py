#!/usr/bin/env python3
"""Profiling aid: one value-and-gradient evaluation of an open-loop rollout (H = 25) timed two ways in ONE process on cuda:0 — HIP
events on the launch stream, alternating windows, the discipline of scripts/time_rollout_vjp.py:

  (a) composed   25 eb_rollout_step launches that keep every pre-step obs, then eb_rollout_chain_vjp (25 reverse launches):
                 what a user had to do before eb_rollout_tape_vjp existed;
  (b) one launch eb_rollout_tape_vjp (csrc/eb_rollout_tape_vjp.hip), and its value-only form;
  (c) context    the forward tape alone, eb_rollout_tape (what bench.py --open-loop times);
  (d) solver     one OpenLoopMPC.solve: us per iteration, launches per iteration.

Information bytes of (b): obs0 in (4 D), the tape in and its gradient out (2 x 8 H), out5 out (20 H) per env.
Every GPU step of a job that calls this runs under its own `timeout`; results go to profiles/.

    python scripts/time_tape_vjp.py [--shapes 65536x32,4096x16] [--iters 20] [--windows 5] [--solver-iterations 10]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd.grad import DifferentiableEnvironmentModel
from env_build_amd.mpc import OpenLoopMPC
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left'); ap.add_argument('--shapes', default='65536x32,4096x16', help='n_env x n_veh, comma separated')
ap.add_argument('--horizon', type=int, default=25); ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--windows', type=int, default=5); ap.add_argument('--solver-iterations', type=int, default=10)
a = ap.parse_args()
dev = torch.device('cuda', 0)
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
H = a.horizon
for shape in a.shapes.split(','):
    n_env, n_veh = (int(v) for v in shape.split('x'))
    inp = make_rollout_inputs(a.task, n_env, n_veh, H, seed=0)
    m = DifferentiableEnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                                   0, ref_indexes=ref).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    tape = torch.from_numpy(inp['actions']).to(dev)
    D, nd = obs0.shape[1], 9
    st = torch.cuda.current_stream(); sp = C.c_void_p(st.cuda_stream)
    lib, h = m.api.lib, m.handle
    step_fn, chain_fn, tape_fn, vjp_fn = lib.eb_rollout_step, m.api.grad_fn('eb_rollout_chain_vjp'), lib.eb_rollout_tape, m.api.grad_fn('eb_rollout_tape_vjp')
    w5 = (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0)
    g5 = torch.tensor([-1.0, 10.0, 0.0, 0.0, 0.0], device=dev).view(1, 5, 1).expand(H, 5, n_env).contiguous()
    steps = torch.empty((H + 1, n_env, D), device=dev); steps[0] = obs0
    out5 = torch.empty((H, 5, n_env), device=dev)
    work, g0, gt = torch.empty((n_env, nd), device=dev), torch.empty((n_env, nd), device=dev), torch.empty((H, n_env, 2), device=dev)
    wk, fin = torch.empty_like(obs0), torch.empty_like(obs0)
    ok = lambda rc: (_ for _ in ()).throw(RuntimeError(lib.eb_last_error())) if rc else None
    def composed():
        for t in range(H):
            ok(step_fn(h, n_env, p(steps[t]), p(tape[t]), p(ref), 0, p(steps[t + 1]), p(out5[t]), None, sp))
        ok(chain_fn(h, n_env, H, p(steps), p(tape), p(ref), 0, None, 0, p(g5), p(work), p(g0), p(gt), sp))
    def one_launch():
        ok(vjp_fn(h, n_env, H, p(obs0), p(tape), p(ref), 0, None, 0, None, w5, p(out5), None, p(g0), p(gt), sp))
    def value_only():
        ok(vjp_fn(h, n_env, H, p(obs0), p(tape), p(ref), 0, None, 0, None, w5, p(out5), None, None, None, sp))
    def forward_tape():
        ok(tape_fn(h, n_env, H, p(obs0), p(tape), p(ref), 0, p(wk), p(fin), p(out5), sp))
    fns = dict(composed=composed, one_launch=one_launch, value_only=value_only, forward_tape=forward_tape)
    for f in fns.values():
        for _ in range(3): f()
    torch.cuda.synchronize()
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters): fn()
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    times = {k: [] for k in fns}
    for _ in range(a.windows):
        for k, f in fns.items(): times[k].append(window(f))
    med = lambda v: sorted(v)[len(v) // 2]
    us = {k: med(v) for k, v in times.items()}
    info_bytes = (4 * D + 16 * H + 20 * H) * n_env
    composed_bytes = H * ((104 + 32 * n_veh) + 4 * D + 8 + 4 * nd + 20 + 4 * nd + 8) * n_env
    # one solve: us per iteration from two solves of different length (the first evaluation and the allocations cancel)
    mpc = OpenLoopMPC(m, horizon=H)
    def solve_us(iters):
        mpc.solve(obs0, ref_indexes=ref, iterations=iters)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); _u, _J, info = mpc.solve(obs0, ref_indexes=ref, iterations=iters); e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, info
    k = a.solver_iterations
    t1, _ = solve_us(k); t2, info = solve_us(2 * k)
    print(json.dumps(dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, iters=a.iters,
                          composed_us=round(us['composed'], 1), composed_us_windows=[round(v, 1) for v in times['composed']],
                          one_launch_us=round(us['one_launch'], 1), one_launch_us_windows=[round(v, 1) for v in times['one_launch']],
                          value_only_us=round(us['value_only'], 1), forward_tape_us=round(us['forward_tape'], 1),
                          composed_over_one_launch=round(us['composed'] / us['one_launch'], 2),
                          one_launch_over_forward_tape=round(us['one_launch'] / us['forward_tape'], 2),
                          one_launch_info_bytes=info_bytes, one_launch_TBps=round(info_bytes / us['one_launch'] / 1e6, 3),
                          one_launch_pct_of_8TBs=round(info_bytes / us['one_launch'] / 1e6 / 8 * 100, 2),
                          composed_alg_bytes=composed_bytes, launches_composed=2 * H, launches_one=1,
                          solver_us_per_iteration=round((t2 - t1) / k, 1), solver_launches_per_iteration=info['launches_per_iteration'],
                          solver_solve_us=round(t2, 1), solver_iterations=2 * k)), flush=True)
