#!/usr/bin/env python3
"""Profiling aid: prioritised replay on the device (include/envbuild_per.h) at one minibatch size `m` over a ring of `capacity` rows of
41 + 2 floats — in ONE process on cuda:0 (one process per shape: run it once per m, with --append), HIP events on the launch stream,
alternating windows, median with spread (the discipline of scripts/time_offpolicy.py).  Per call:

  (uniform_sample)   the baseline: eb_replay_sample, keyed route, the five outputs of a SAC minibatch and the noise ids, one launch
  (per_sample)       eb_per_sample (index, priority, noise id, the 64 minima) + eb_replay_sample with those indices: two launches
  (per_draw)         eb_per_sample alone
  (set_indexed)      eb_per_set, indexed route, m rows as a draw left them: eb_per_set_launches(C, indexed) launches
  (set_range)        eb_per_set, range route, m rows at a cursor that wraps: eb_per_set_launches(C, range) launches
  (sac_graph)        the baseline: a replayed offpolicy.SAC graph, policy 41 -> 2 x 256 -> 4, critics 43 -> 2 x 256 -> 1, uniform draws
  (per_sac_graph)    a replayed per.SAC graph on the same ring, networks of the same shapes and seeds, over the same tree

The priorities are spread over four decades with a quarter of the leaves at max_prio, as after some training.  Timing is recorded, not
asserted, and no ratio is promised.  What the figures do not show: whether the tree's upper levels and the leaves sat in the Infinity
Cache between calls (the windows repeat one call back to back, so they largely do), and no roofline is claimed — the descent is a chain of
dependent loads, latency-bound, not bandwidth-bound.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_per.py [--m 4096] [--capacity 1048576] [--windows 20] [--iters 20] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import offpolicy as O
from env_build_amd import per as P
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--m', type=int, default=4096); ap.add_argument('--capacity', type=int, default=1 << 20)
ap.add_argument('--windows', type=int, default=20); ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r31_per_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)
M, CAP, D, A, H = a.m, a.capacity, 41, 2, 256
gen = torch.Generator(device=dev); gen.manual_seed(0)
rnd = lambda *s: torch.randn(s, device=dev, generator=gen)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def fill(buf):
    buf.obs.copy_(rnd(CAP, D)); buf.next_obs.copy_(rnd(CAP, D)); buf.act.copy_(torch.tanh(rnd(CAP, A))); buf.rew.copy_(rnd(CAP))
    buf.nonterminal.copy_((torch.rand(CAP, device=dev, generator=gen) < 0.98).float())
    buf.fill.fill_(CAP); buf.size = CAP


def nets(seed):
    return (TrainableMLPNet(D, 2, H, 'elu', 2 * A, output_activation='linear', device=dev, seed=seed),
            TrainableMLPNet(D + A, 2, H, 'elu', 1, output_activation='linear', device=dev, seed=seed + 1),
            TrainableMLPNet(D + A, 2, H, 'elu', 1, output_activation='linear', device=dev, seed=seed + 2))


# ---- the two rings: the same transitions; the prioritised one with every leaf set ----
plain, pri = O.ReplayBuffer(CAP, D, A, dev), P.PrioritizedReplayBuffer(CAP, D, A, dev)
fill(plain)
for k in ('obs', 'act', 'rew', 'next_obs', 'nonterminal'):
    getattr(pri, k).copy_(getattr(plain, k))
pri.fill.fill_(CAP); pri.size = CAP
P.set_range(pri, 0, CAP)
spread = torch.exp(torch.rand(CAP, device=dev, generator=gen) * float(np.log(1e4)) + float(np.log(1e-2)))
some = torch.nonzero(torch.rand(CAP, device=dev, generator=gen) < 0.75).squeeze(1).to(torch.int32)
pri.update_priorities(some, spread[some.long()].contiguous())
torch.cuda.synchronize()
off, per = O.offpolicy_api(), P.per_api()
rows = lambda: dict(obs=torch.empty(M, D, device=dev), qin=torch.empty(M, D + A, device=dev), next_obs=torch.empty(M, D, device=dev),
                    rew=torch.empty(M, device=dev), nonterminal=torch.empty(M, device=dev), noise_id=torch.zeros(M, dtype=torch.int32, device=dev))
mb_u, mb_p = rows(), rows()
mb_p.update(index=torch.zeros(M, dtype=torch.int32, device=dev), prio=torch.empty(M, device=dev))
partials = torch.empty(P.EB_PER_MIN_BLOCKS, device=dev)
u_args = plain.sample_args(mb_u, seed=1, draw=0)
d_args = pri.draw_args(mb_p['index'], mb_p['prio'], mb_p['noise_id'], partials, seed=1, draw=0)
g_args = pri.gather_args(mb_p, seed=1, draw=0)
value = torch.exp(rnd(M)).contiguous()
per.check(per.sample(C.byref(d_args)))                                             # the indices the write-back names: a draw's own
x_args = pri.set_args(P.EB_PER_ROUTE_INDEXED, M, index=mb_p['index'], value=value)
r_args = pri.set_args(P.EB_PER_ROUTE_RANGE, min(M, CAP), start=CAP - min(M, CAP) // 2)
for s in (u_args, d_args, g_args, x_args, r_args):
    s.stream = st.cuda_stream


def uniform_sample(): off.check(off.sample(C.byref(u_args)))
def per_draw(): per.check(per.sample(C.byref(d_args)))
def per_sample(): per.check(per.sample(C.byref(d_args))); off.check(off.sample(C.byref(g_args)))
def set_indexed(): per.check(per.set(C.byref(x_args)))
def set_range(): per.check(per.set(C.byref(r_args)))


# ---- the two updates ----
sac = O.SAC(*nets(0), plain, M, gamma=0.99, tau=0.005, lr=3e-4, seed=0)
psac = P.SAC(*nets(0), pri, M, alpha=0.6, beta0=0.4, beta_step=1e-4, eps=1e-6, gamma=0.99, tau=0.005, lr=3e-4, seed=0)
graph, pgraph = sac.capture(), psac.capture()
routes = {'uniform_sample': uniform_sample, 'per_sample': per_sample, 'per_draw': per_draw, 'set_indexed': set_indexed, 'set_range': set_range,
          'sac_graph': lambda: sac.replay(graph), 'per_sac_graph': lambda: psac.replay(pgraph)}
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn, a.iters))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='per', m=M, capacity=CAP, obs_dim=D, act_dim=A, hidden=H, windows=a.windows, iters=a.iters, levels=len(P.tree_levels(CAP)[0]) - 1,
           set_launches_indexed=pri.launches(P.EB_PER_ROUTE_INDEXED), set_launches_range=pri.launches(P.EB_PER_ROUTE_RANGE),
           sac_kernels=O.SAC.KERNELS, per_sac_kernels=psac.KERNELS, unit='us per call, median of the windows')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_spread_us'] = r(max(times[k]) - min(times[k])); rec[k + '_min_us'] = r(min(times[k]))
rec['per_sample_over_uniform'] = round(us['per_sample'] / us['uniform_sample'], 2)
rec['per_sac_over_sac'] = round(us['per_sac_graph'] / us['sac_graph'], 3)
torch.cuda.synchronize()
tree, prio = pri.tree.cpu().numpy(), pri.prio.cpu().numpy()
rec['invariant'] = bool(np.array_equal(tree, P.tree_reference(prio)))              # after all of the above the tree is still the rebuild
rec['finite'] = bool(all(np.isfinite(v) for v in psac.log().values()) and all(np.isfinite(v) for v in sac.log().values()))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
