#!/usr/bin/env python3
"""Profiling aid: the stochastic policy head (csrc/eb_policy_sample.hip) at 65 536 x (137 -> 256 -> 256 -> 4), elu hidden, linear out,
scale set, action_range 1, in ONE process on cuda:0, HIP events on the launch stream, alternating windows (the discipline of
scripts/time_policy_f16.py).  Four ways to a batch of actions:

  (fused)     eb_policy_sample: network, drawn noise, actions and logp in one launch;
  (mode)      eb_policy_run_batch: the deterministic action, what the fused launch adds its epilogue to;
  (composed)  eb_mlp_forward followed by eb_policy_sample_from_logits: two launches, the logits through memory;
  (torch)     eb_mlp_forward followed by torch's TransformedDistribution(Independent(Normal), [Tanh, Affine]).rsample / log_prob:
              the only route there was before the entry existed.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_sample.py [--n 65536] [--iters 200] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from torch import distributions as D
from env_build_amd import policy_sample as ps
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.policy import MLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=65536); ap.add_argument('--obs-dim', type=int, default=137)
ap.add_argument('--iters', type=int, default=200); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r19_policy_sample_timing.txt'))
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
p = lambda t: t.data_ptr() if t is not None else None

n, obs_dim = a.n, a.obs_dim
rng = np.random.default_rng(0)
net = MLPNet(obs_dim, 2, 256, 'elu', 4, device=dev)
net.set_obs_scale(rng.uniform(0.02, 0.2, obs_dim).astype(np.float32))
obs = torch.from_numpy((rng.standard_normal((n, obs_dim)) * 10).astype(np.float32)).to(dev)
actions = torch.empty((n, 2), dtype=torch.float32, device=dev)
logp = torch.empty((n,), dtype=torch.float32, device=dev)
logits = torch.empty((n, 4), dtype=torch.float32, device=dev)
fns = ps.bind(net.api)
h, s = net._handle, _stream(dev)
count = [0]


def fused():
    count[0] += 1
    net.api.check(fns['eb_policy_sample'](h, n, p(obs), None, None, 0, count[0], 1.0, p(actions), p(logp), None, None, s))


def mode():
    net.api.policy_run_batch(h, n, C.c_void_p(p(obs)), C.c_float(1.0), C.c_void_p(p(actions)), s)


def composed():
    count[0] += 1
    net.api.mlp_forward(h, n, C.c_void_p(p(obs)), C.c_void_p(p(logits)), s)
    net.api.check(fns['eb_policy_sample_from_logits'](n, 4, p(logits), None, None, 0, count[0], 1.0, p(actions), p(logp), None, s))


def with_torch():
    net.api.mlp_forward(h, n, C.c_void_p(p(obs)), C.c_void_p(p(logits)), s)
    dist = D.TransformedDistribution(D.Independent(D.Normal(logits[:, :2], logits[:, 2:].exp()), 1),
                                     [D.transforms.TanhTransform(cache_size=1), D.transforms.AffineTransform(0.0, 1.0, cache_size=1)])
    act = dist.rsample()
    return act, dist.log_prob(act)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


routes = {'fused': fused, 'mode': mode, 'composed': composed, 'torch': with_torch}
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='policy_sample', n=n, net='%d -> 256 -> 256 -> 4, elu / linear, scale set, action_range 1' % obs_dim, iters=a.iters)
for k in routes:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
rec['fused_over_mode'] = round(us['fused'] / us['mode'], 3)
rec['composed_over_fused'] = round(us['composed'] / us['fused'], 3)
rec['torch_over_fused'] = round(us['torch'] / us['fused'], 3)
# the fused launch and the composed pair give the same bits
fused(); torch.cuda.synchronize(); a1, l1 = actions.clone(), logp.clone()
count[0] -= 1; composed(); torch.cuda.synchronize()
rec['fused_equals_composed'] = bool(torch.equal(a1, actions) and torch.equal(l1, logp))
line = json.dumps(rec)
print(line, flush=True)
lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
