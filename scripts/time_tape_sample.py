#!/usr/bin/env python3
"""Profiling aid: one MPPI step — S perturbed tapes per env drawn, scored and soft-min averaged (H = 25) — two ways in ONE process
on cuda:0, HIP events on the launch stream, alternating windows, the discipline of scripts/time_tape_cand.py:

  (new)    one eb_rollout_tape_sample launch (csrc/eb_rollout_tape_sample.hip) with cost, best and mean;
  (today)  what a caller could do before: torch-generated tapes [S, H, B, 2] (randn, scale, add, clamp), ceil(S / tape_cand_max)
           eb_rollout_tape_cand launches for the costs, then the soft-min average and the best tape in torch.

Before timing, the costs of the new launch are checked to be the bits of the candidate path over the tapes it dumps.  Every GPU step
of a job that calls this runs under its own `timeout`.

    python scripts/time_tape_sample.py [--shapes 4096x16x64,4096x16x256,4096x16x1024,65536x32x64] [--iters 20] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from env_build_amd.cand import tape_cand_max
from env_build_amd.dynamics_and_models import EnvironmentModel
from env_build_amd.synthetic import make_rollout_inputs

ap = argparse.ArgumentParser()
ap.add_argument('--task', default='left')
ap.add_argument('--shapes', default='4096x16x64,4096x16x256,4096x16x1024,65536x32x64', help='n_env x n_veh x n_samples, comma separated')
ap.add_argument('--horizon', type=int, default=25); ap.add_argument('--iters', type=int, default=20); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r11_tape_sample_timing.txt'))
a = ap.parse_args()
dev = torch.device('cuda', 0)
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
H = a.horizon
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
for shape in a.shapes.split(','):
    n_env, n_veh, S = (int(v) for v in shape.split('x'))
    torch.cuda.reset_peak_memory_stats(dev)
    inp = make_rollout_inputs(a.task, n_env, n_veh, H, seed=0)
    m = EnvironmentModel(a.task, 0, mode='training', n_veh=n_veh, device=dev)
    ego = torch.from_numpy(inp['ego']).to(dev); ref = torch.from_numpy(inp['ref_idx']).to(dev)
    trk = m.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(), ego[:, 0].contiguous(),
                                                   0, ref_indexes=ref).t
    obs0 = torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous()
    nominal = torch.from_numpy(inp['actions']).to(dev).clamp(-1, 1).contiguous()
    st = torch.cuda.current_stream(); sp = C.c_void_p(st.cuda_stream)
    lib, h = m.api.lib, m.handle
    s_fn, c_fn = m.api.sample_fn('eb_rollout_tape_sample'), m.api.cand_fn('eb_rollout_tape_cand')
    w5 = (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0); sig = (C.c_float * 2)(0.3, 0.3)
    sigma = torch.tensor([0.3, 0.3], device=dev)
    inv_lambda = 0.5
    ok = lambda rc: (_ for _ in ()).throw(RuntimeError(lib.eb_last_error())) if rc else None
    limit = tape_cand_max(m, H)
    cost = torch.empty((S, n_env), device=dev); best_tape = torch.empty((H, n_env, 2), device=dev); best_cost = torch.empty(n_env, device=dev)
    best_index = torch.empty(n_env, dtype=torch.int32, device=dev); mean_tape = torch.empty((H, n_env, 2), device=dev)
    counter = [0]
    def new(dump=None):
        counter[0] += 1
        ok(s_fn(h, n_env, S, H, p(obs0), p(nominal), p(ref), 0, None, 1, counter[0], sig, 0.0, inv_lambda, w5, p(cost), p(best_tape), p(best_cost),
                p(best_index), p(mean_tape), p(dump), sp))
    cost_t = torch.empty((S, n_env), device=dev)
    def cand_costs(tapes):
        for k0 in range(0, S, limit):
            k1 = min(S, k0 + limit)
            ok(c_fn(h, n_env, k1 - k0, H, p(obs0), p(tapes[k0:k1]), p(ref), 0, None, 0, 0, w5, None, p(cost_t[k0:k1]), sp))
    gen = torch.Generator(device=dev).manual_seed(0)
    def today():
        tapes = torch.randn((S, H, n_env, 2), device=dev, generator=gen).mul_(sigma).add_(nominal)
        tapes[0] = nominal
        tapes.clamp_(-1.0, 1.0)
        cand_costs(tapes)
        lo, idx = cost_t.min(0)
        w = torch.exp((lo - cost_t) * inv_lambda)
        mean = ((w.view(S, 1, n_env, 1) * tapes).sum(0) / w.sum(0).view(1, n_env, 1)).clamp_(-1.0, 1.0)
        best = tapes.gather(0, idx.view(1, 1, n_env, 1).expand(1, H, n_env, 2))[0]
        return mean, best, lo
    # the new launch's costs are the candidate path's bits over the tapes it scored (the timing compares like with like)
    dump = torch.empty((S, H, n_env, 2), device=dev)
    new(dump); cand_costs(dump); torch.cuda.synchronize()
    assert torch.equal(cost.view(torch.int32), cost_t.view(torch.int32)), 'the new launch and the candidate path disagree'
    del dump
    for _ in range(3):
        new(); today()
    torch.cuda.synchronize()
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters): fn()
        e1.record(st); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters
    times = dict(new=[], today=[])
    for _ in range(a.windows):
        times['new'].append(window(new)); times['today'].append(window(today))
    r = lambda v: round(v, 1)
    us = {k: med(v) for k, v in times.items()}
    tape_bytes = S * H * n_env * 2 * 4
    line = json.dumps(dict(task=a.task, n_env=n_env, n_veh=n_veh, horizon=H, n_samples=S, tape_cand_max=limit, cand_launches_today=-(-S // limit),
                           iters=a.iters, new_us=r(us['new']), new_us_windows=[r(v) for v in times['new']], today_us=r(us['today']),
                           today_us_windows=[r(v) for v in times['today']], today_spread_us=r(spread(times['today'])),
                           gain_us=r(us['today'] - us['new']), today_over_new=round(us['today'] / us['new'], 2),
                           faster_by_more_than_the_spread=bool(us['today'] - us['new'] > spread(times['today'])),
                           tape_bytes_not_allocated=tape_bytes, torch_peak_bytes_today=int(torch.cuda.max_memory_allocated(dev))))
    print(line, flush=True)
    lines.append(line)
    del cost, cost_t, m
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
