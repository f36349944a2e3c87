#!/usr/bin/env python3
"""Profiling aid: off-policy training on the device (include/envbuild_offpolicy.h) at one minibatch size `m` over a ring of `capacity`
rows of 41 + 2 floats — in ONE process on cuda:0 (one process per shape: run it once per m, with --append), HIP events on the launch
stream, alternating windows, median with spread (the discipline of scripts/time_collect.py).  Per call:

  (push_4096, push_65536)  eb_replay_push of that many rows, both parts, final observations given, at a cursor that wraps
  (sample)                 eb_replay_sample: the five outputs of a SAC minibatch and the noise ids, keyed route, one launch
  (torch_sample)           a torch twin: torch.randint and five index_selects into preallocated outputs
  (sac_graph)              a replayed offpolicy.SAC graph: policy 41 -> 2 x 256 -> 4, critics 43 -> 2 x 256 -> 1
  (torch_sac)              a torch twin of the same update on the same shapes: torch.nn modules, torch.optim.Adam (capturable),
                           torch.lerp_ for the targets, its own randint + index_select sampling, captured with torch.cuda.graph where
                           torch allows it (`torch_sac_captured` says whether it did)

Timing is recorded, not asserted, and no ratio is promised.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_offpolicy.py [--m 4096] [--capacity 1048576] [--windows 20] [--iters 20] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import offpolicy as O
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--m', type=int, default=4096); ap.add_argument('--capacity', type=int, default=1 << 20)
ap.add_argument('--windows', type=int, default=20); ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r30_offpolicy_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)
M, CAP, D, A, H = a.m, a.capacity, 41, 2, 256
GAMMA, TAU, LR = 0.99, 0.005, 3e-4
gen = torch.Generator(device=dev); gen.manual_seed(0)
rnd = lambda *s: torch.randn(s, device=dev, generator=gen)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


# ---- the ring, full of synthetic transitions ----
buf = O.ReplayBuffer(CAP, D, A, dev)
buf.obs.copy_(rnd(CAP, D)); buf.next_obs.copy_(rnd(CAP, D)); buf.act.copy_(torch.tanh(rnd(CAP, A))); buf.rew.copy_(rnd(CAP))
buf.nonterminal.copy_((torch.rand(CAP, device=dev, generator=gen) < 0.98).float())
buf.fill.fill_(CAP); buf.size = CAP
api = O.offpolicy_api()
pushes = {}
for n in (4096, 65536):
    if n > CAP: continue
    src = dict(prev_obs=rnd(n, D), action=rnd(n, A), reward=rnd(n), obs_after=rnd(n, D), final_obs=rnd(n, D),
               done_code=(torch.randint(0, 8, (n,), device=dev, generator=gen) * (torch.rand(n, device=dev, generator=gen) < 0.05)).to(torch.uint8))
    p = buf.push_args(n)
    p.start, p.fill_after, p.stream = CAP - n // 2, CAP, st.cuda_stream             # the batch wraps
    for k, t in src.items(): setattr(p, k, t.data_ptr())
    pushes[n] = (p, src)
mb = dict(obs=torch.empty(M, D, device=dev), qin=torch.empty(M, D + A, device=dev), next_obs=torch.empty(M, D, device=dev),
          rew=torch.empty(M, device=dev), nonterminal=torch.empty(M, device=dev), noise_id=torch.zeros(M, dtype=torch.int32, device=dev))
s_args = buf.sample_args(mb, seed=1, draw=0)
s_args.stream = st.cuda_stream
t_out = dict(obs=torch.empty(M, D, device=dev), act=torch.empty(M, A, device=dev), next_obs=torch.empty(M, D, device=dev),
             rew=torch.empty(M, device=dev), nonterminal=torch.empty(M, device=dev))
t_idx = torch.zeros(M, dtype=torch.int64, device=dev)


def sample(): api.check(api.sample(C.byref(s_args)))


def torch_sample():
    torch.randint(0, CAP, (M,), device=dev, out=t_idx)
    for k, out in t_out.items():
        torch.index_select(getattr(buf, k), 0, t_idx, out=out)


# ---- the update ----
policy = TrainableMLPNet(D, 2, H, 'elu', 2 * A, output_activation='linear', device=dev, seed=0)
q1 = TrainableMLPNet(D + A, 2, H, 'elu', 1, output_activation='linear', device=dev, seed=1)
q2 = TrainableMLPNet(D + A, 2, H, 'elu', 1, output_activation='linear', device=dev, seed=2)
sac = O.SAC(policy, q1, q2, buf, M, gamma=GAMMA, tau=TAU, lr=LR, seed=0)
graph = sac.capture()


def sac_graph(): sac.replay(graph)


def mlp(i, o):
    return torch.nn.Sequential(torch.nn.Linear(i, H), torch.nn.ELU(), torch.nn.Linear(H, H), torch.nn.ELU(), torch.nn.Linear(H, o)).to(dev)


t_pi, t_q = mlp(D, 2 * A), [mlp(D + A, 1), mlp(D + A, 1)]
t_qt = [mlp(D + A, 1), mlp(D + A, 1)]
for q, t in zip(t_q, t_qt): t.load_state_dict(q.state_dict())
t_la = torch.zeros(1, device=dev, requires_grad=True)
opts = [torch.optim.Adam(n.parameters(), lr=LR, capturable=True) for n in (t_q[0], t_q[1], t_pi)] + [torch.optim.Adam([t_la], lr=LR, capturable=True)]
LOG2, HALF_LOG_2PI = float(np.log(2.0)), float(0.5 * np.log(2 * np.pi))


def draw(net, obs):
    mean, ls = net(obs).split(A, dim=1)
    eps = torch.randn_like(mean)
    u = mean + ls.exp() * eps
    logp = (-0.5 * eps * eps - ls - HALF_LOG_2PI).sum(1) - (2.0 * (LOG2 - u - torch.nn.functional.softplus(-2.0 * u))).sum(1)
    return torch.tanh(u), logp


def torch_sac():
    idx = torch.randint(0, CAP, (M,), device=dev)
    obs, act, nxt = buf.obs.index_select(0, idx), buf.act.index_select(0, idx), buf.next_obs.index_select(0, idx)
    rew, nt = buf.rew.index_select(0, idx), buf.nonterminal.index_select(0, idx)
    with torch.no_grad():
        a2, lp2 = draw(t_pi, nxt)
        x2 = torch.cat([nxt, a2], 1)
        y = rew + GAMMA * nt * (torch.minimum(t_qt[0](x2), t_qt[1](x2)).squeeze(1) - t_la.exp() * lp2)
    x = torch.cat([obs, act], 1)
    for q, opt in zip(t_q, opts[:2]):
        opt.zero_grad(set_to_none=True)
        (0.5 * (q(x).squeeze(1) - y) ** 2).mean().backward()
        opt.step()
    a1, lp = draw(t_pi, obs)
    x1 = torch.cat([obs, a1], 1)
    for q in t_q: q.requires_grad_(False)
    opts[2].zero_grad(set_to_none=True)
    (t_la.exp().detach() * lp - torch.minimum(t_q[0](x1), t_q[1](x1)).squeeze(1)).mean().backward()
    opts[2].step()
    for q in t_q: q.requires_grad_(True)
    opts[3].zero_grad(set_to_none=True)
    (-(t_la * (lp.detach() - float(A)).mean())).backward()
    opts[3].step()
    with torch.no_grad():
        for q, t in zip(t_q, t_qt):
            for p, pt in zip(q.parameters(), t.parameters()): pt.lerp_(p, TAU)


captured = False
try:
    side = torch.cuda.Stream()
    side.wait_stream(st)
    with torch.cuda.stream(side):
        for _ in range(3): torch_sac()
    st.wait_stream(side); torch.cuda.synchronize()
    t_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(t_graph):
        torch_sac()
    run_torch_sac, captured = t_graph.replay, True
except Exception as e:   # noqa: BLE001
    print('# the torch twin was not captured (%s: %s): timed eagerly' % (type(e).__name__, str(e).splitlines()[0][:160]), flush=True)
    torch.cuda.synchronize()
    run_torch_sac = torch_sac

routes = {'sample': sample, 'torch_sample': torch_sample, 'sac_graph': sac_graph, 'torch_sac': run_torch_sac}
for n, (p, _src) in pushes.items():
    routes['push_%d' % n] = (lambda p=p: api.check(api.push(C.byref(p))))
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn, a.iters))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='offpolicy', m=M, capacity=CAP, obs_dim=D, act_dim=A, hidden=H, windows=a.windows, iters=a.iters, sac_kernels=O.SAC.KERNELS,
           torch_sac_captured=captured, unit='us per call, median of the windows')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_spread_us'] = r(max(times[k]) - min(times[k])); rec[k + '_min_us'] = r(min(times[k]))
rec['sample_bytes'] = 4 * M * (2 * D + (D + A) + 4) * 2
rec['sample_GBps'] = r(rec['sample_bytes'] / us['sample'] / 1e3)
for n in pushes:
    rec['push_%d_GBps' % n] = r(2 * 4 * n * (3 * D + A + 2) / us['push_%d' % n] / 1e3)
torch.cuda.synchronize()
rec['finite'] = bool(all(np.isfinite(v) for v in sac.log().values()))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
