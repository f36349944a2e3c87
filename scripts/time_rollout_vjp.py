#!/usr/bin/env python3
"""Profiling aid: kernel-only timing of eb_rollout_step (forward) and eb_rollout_step_vjp (reverse) in ONE process on cuda:0 —
HIP events on the launch stream, the warm-up / repeat discipline of scripts/time_rollout.py.  The comparison that counts is
reverse against forward of the same run; the two are timed in alternating windows.

Algorithmic bytes per env-step (fp32, D = nd + 4 * n_veh, nd = 6 + 3 * (n_future + 1)):
  forward  104 + 32 * n_veh + 24 * n_future                    (scripts/time_rollout.py)
  reverse  (4 D + 8) read obs, actions + (4 nd + 20) read cotangents + (4 nd + 8) written   (compact rows, ld_in == nd)"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd.grad import DifferentiableEnvironmentModel
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left'); ap.add_argument('--mode', default='training'); ap.add_argument('--n-future', type=int, default=0)
ap.add_argument('--shapes', default='65536x32,4096x16', help='n_env x n_veh, comma separated')
ap.add_argument('--iters', type=int, default=200); ap.add_argument('--windows', type=int, default=5, help='timed windows per direction, alternating')
ap.add_argument('--full-rows', action='store_true', help='ld_in == D: the launch also zero-fills the vehicle columns (what the autograd facade asks for)')
a = ap.parse_args()
dev = torch.device('cuda', 0)
p = lambda t: C.c_void_p(t.data_ptr())
for shape in a.shapes.split(','):
    n_env, n_veh = (int(v) for v in shape.split('x'))
    inp = make_rollout_inputs(a.task, n_env, n_veh, 25, seed=0)
    m = DifferentiableEnvironmentModel(a.task, a.n_future, mode=a.mode, n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    if a.mode != 'training': m.ref_path.set_path(1)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                                   a.n_future, ref_indexes=ref if a.mode == 'training' else None).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    tape = torch.from_numpy(inp['actions']).to(dev)
    D, nd = obs0.shape[1], 9 + 3 * a.n_future
    st = torch.cuda.current_stream(); sp = C.c_void_p(st.cuda_stream)
    rp = p(ref) if a.mode == 'training' else None
    # forward: a 25-step rollout kept whole (its pre-step obs are the reverse pass's inputs)
    states = [obs0] + [torch.empty_like(obs0) for _ in range(25)]
    out5 = torch.empty((25, 5, n_env), device=dev)
    fwd_fn, vjp_fn = m.api.lib.eb_rollout_step, m.api.grad_fn('eb_rollout_step_vjp')
    def fwd(i):
        t = i % 25
        rc = fwd_fn(m.handle, n_env, p(states[t]), p(tape[t]), rp, 1, p(states[t + 1]), p(out5[t]), None, sp)
        assert rc == 0, m.api.lib.eb_last_error()
    g = torch.Generator(device=dev).manual_seed(0)
    g5 = torch.randn((5, n_env), device=dev, generator=g)
    ld_in = D if a.full_rows else nd
    gbuf = [torch.randn((n_env, nd), device=dev, generator=g), torch.empty((n_env, nd), device=dev)] if not a.full_rows else \
           [torch.randn((n_env, D), device=dev, generator=g), torch.empty((n_env, D), device=dev)]
    gact = torch.empty((25, n_env, 2), device=dev)
    def vjp(i):
        t = 24 - i % 25                            # last step first, cotangent rows ping-pong as in eb_rollout_chain_vjp
        rc = vjp_fn(m.handle, n_env, p(states[t]), p(tape[t]), rp, 1, p(gbuf[i & 1]), ld_in, p(g5), p(gbuf[(i & 1) ^ 1]), ld_in, p(gact[t]), sp)
        assert rc == 0, m.api.lib.eb_last_error()
    for i in range(50): fwd(i)
    for i in range(50): vjp(i)
    torch.cuda.synchronize()
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for i in range(a.iters): fn(i)
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    tf_, tv_ = [], []
    for _ in range(a.windows):
        gbuf[0].normal_(generator=g)              # (a 200-step product of Jacobians would overflow: a fresh cotangent per window)
        tf_.append(window(fwd)); tv_.append(window(vjp))
    med = lambda v: sorted(v)[len(v) // 2]
    bytes_f = (104 + 32 * n_veh + 24 * a.n_future) * n_env
    bytes_v = ((4 * D + 8) + (4 * nd + 20) + (4 * nd + 8)) * n_env
    uf, uv = med(tf_), med(tv_)
    print(json.dumps(dict(task=a.task, mode=a.mode, n_env=n_env, n_veh=n_veh, n_future=a.n_future, full_rows=bool(a.full_rows), iters=a.iters,
                          forward_us=round(uf, 2), forward_us_windows=[round(v, 2) for v in tf_], forward_alg_bytes=bytes_f,
                          forward_pct_of_8TBs=round(bytes_f / uf / 1e6 / 8 * 100, 1),
                          vjp_us=round(uv, 2), vjp_us_windows=[round(v, 2) for v in tv_], vjp_alg_bytes=bytes_v,
                          vjp_pct_of_8TBs=round(bytes_v / uv / 1e6 / 8 * 100, 1), vjp_over_forward=round(uv / uf, 3))))
