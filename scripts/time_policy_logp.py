#!/usr/bin/env python3
"""Profiling aid: the log-probability of given actions (csrc/eb_policy_logp.hip) at n x (obs_dim -> 256 -> 256 -> 4), elu hidden, linear
out, scale set, action_range 1, in ONE process on cuda:0, HIP events on the launch stream, alternating windows (the discipline of
scripts/time_policy_sample.py).  Four ways to logp of stored actions:

  (fused)     eb_policy_logp: network and epilogue in one launch;
  (sample)    eb_policy_sample at the same shape: what the fused launch is expected to cost;
  (composed)  eb_mlp_forward followed by eb_policy_logp_from_logits: two launches, the logits through memory;
  (torch)     a TrainableMLPNet forward (no graph) followed by torch's TransformedDistribution(Independent(Normal), [Tanh, Affine])
              .log_prob(actions): the only route there was before the entry existed;

and forward + backward of the training surface: policy_logp.log_prob against the same distribution on TrainableMLPNet.call's logits
(both end in one eb_mlp_backward).  Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own
`timeout`.

    python scripts/time_policy_logp.py [--n 65536] [--obs-dim 137] [--iters 200] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from torch import distributions as D
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=65536); ap.add_argument('--obs-dim', type=int, default=137)
ap.add_argument('--iters', type=int, default=200); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r22_policy_logp_timing.txt'))
ap.add_argument('--only', default='', help='comma-separated routes (for a kernel trace of a few)')
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
net = TrainableMLPNet(obs_dim, 2, 256, 'elu', 4, device=dev)
net.set_obs_scale(rng.uniform(0.02, 0.2, obs_dim).astype(np.float32))
obs = torch.from_numpy((rng.standard_normal((n, obs_dim)) * 10).astype(np.float32)).to(dev)
logits = torch.empty((n, 4), dtype=torch.float32, device=dev)
logp = torch.empty((n,), dtype=torch.float32, device=dev)
scratch = torch.empty((n, 2), dtype=torch.float32, device=dev)
actions = ps.sample_actions(net, obs, 1.0, seed=1, want=())['actions'].t.clone()      # stored samples of this policy
g_lp = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
fns, sfns = pl.bind(net.api), ps.bind(net.api)
h, s = net._handle, _stream(dev)
fused_args = pl._args(s, n, 0, 1.0, obs=obs, actions=actions, logp=logp)
alone_args = pl._args(s, n, 4, 1.0, logits=logits, actions=actions, logp=logp)


def fused():
    net.api.check(fns['eb_policy_logp'](h, C.byref(fused_args)))


def sample():
    net.api.check(sfns['eb_policy_sample'](h, n, p(obs), None, None, 0, 1, 1.0, p(scratch), p(logp), None, None, s))


def composed():
    net.api.mlp_forward(h, n, C.c_void_p(p(obs)), C.c_void_p(p(logits)), s)
    net.api.check(fns['eb_policy_logp_from_logits'](C.byref(alone_args)))


def dist_of(y):
    return D.TransformedDistribution(D.Independent(D.Normal(y[:, :2], y[:, 2:].exp()), 1),
                                     [D.transforms.TanhTransform(), D.transforms.AffineTransform(0.0, 1.0)])


def with_torch():
    with torch.no_grad():
        return dist_of(net.call(obs)).log_prob(actions)


def train_fused():
    lp, _ = pl.log_prob(net, obs, actions, 1.0)
    for q in net.parameters():
        q.grad = None
    (lp * g_lp).sum().backward()


def train_torch():
    lp = dist_of(net.call(obs)).log_prob(actions)
    for q in net.parameters():
        q.grad = None
    (lp * g_lp).sum().backward()


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


routes = {'fused': fused, 'sample': sample, 'composed': composed, 'torch': with_torch, 'train_fused': train_fused, 'train_torch': train_torch}
if a.only:
    routes = {k: routes[k] for k in a.only.split(',')}
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='policy_logp', n=n, net='%d -> 256 -> 256 -> 4, elu / linear, scale set, action_range 1' % obs_dim, iters=a.iters)
for k in routes:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
if not a.only:
    rec['fused_over_sample'] = round(us['fused'] / us['sample'], 3)
    rec['composed_over_fused'] = round(us['composed'] / us['fused'], 3)
    rec['torch_over_fused'] = round(us['torch'] / us['fused'], 3)
    rec['train_torch_over_train_fused'] = round(us['train_torch'] / us['train_fused'], 3)
    # the fused launch and the composed pair give the same bits; the torch route the same density
    fused(); torch.cuda.synchronize(); l1 = logp.clone()
    composed(); torch.cuda.synchronize()
    rec['fused_equals_composed'] = bool(torch.equal(l1, logp))
    inside = actions.abs().max(1).values < 1.0             # torch has no clamp: an action on the range has log_prob inf there
    rec['rows_on_the_range'] = int((~inside).sum())
    rec['torch_minus_fused_max'] = float((with_torch() - l1)[inside].abs().max())
line = json.dumps(rec)
print(line, flush=True)
lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
