#!/usr/bin/env python3
"""Profiling aid: the PPO update's arithmetic (csrc/eb_ppo.hip) at n x (obs_dim -> 256 -> 256 -> 4), elu hidden, linear out, scale set,
action_range 1, T = 32 steps of n / 32 envs, in ONE process on cuda:0, HIP events on the launch stream, alternating windows (the
discipline of scripts/time_policy_logp.py).  Three comparisons, both sides of each in this process on this tree:

  (gae / gae_torch)        eb_gae against the reverse loop of examples/ppo_env_loop.py in torch, [T, n / T] arrays;
  (loss / loss_torch)      policy_loss forward + backward against policy_logp.log_prob plus the example's torch expressions (exp,
                           clamp, two products, min, mean, the entropy) forward + backward; both end in one eb_mlp_backward;
  (surrogate / logp)       eb_ppo_surrogate with every output against eb_policy_logp: what the longer row function costs.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_ppo.py [--n 65536] [--obs-dim 137] [--steps 32] [--iters 100] [--windows 5] [--out FILE] [--append] [--gae-envs 1048576]"""
import argparse, ctypes as C, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd import ppo
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=65536); ap.add_argument('--obs-dim', type=int, default=137)
ap.add_argument('--steps', type=int, default=32)
ap.add_argument('--iters', type=int, default=100); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r23_ppo_timing.txt'))
ap.add_argument('--gae-envs', type=int, default=0, help='also time eb_gae alone at this many envs x --steps (a size bound by memory)')
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

n, obs_dim, T = a.n, a.obs_dim, a.steps
B = n // T
gamma, lam, clip, ent_coef = 0.99, 0.95, 0.2, 1e-3
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
net = TrainableMLPNet(obs_dim, 2, 256, 'elu', 4, device=dev)
net.set_obs_scale(rng.uniform(0.02, 0.2, obs_dim).astype(np.float32))
obs = gpu(rng.standard_normal((n, obs_dim)) * 10)
actions = ps.sample_actions(net, obs, 1.0, seed=1, want=())['actions'].t.clone()      # stored samples of this policy
# logp_old a little off the present weights' logp, so that all three regions of the clamp are populated
logp_old = pl.log_prob_actions(net, obs, actions, 1.0)['logp'].t + gpu(rng.uniform(-0.4, 0.4, n))
rew, val, v_last = gpu(rng.standard_normal((T, B))), gpu(rng.standard_normal((T, B))), gpu(rng.standard_normal(B))
live = gpu(rng.uniform(size=(T, B)) > 0.02)
adv_buf, ret_buf = torch.empty((T, B), device=dev), torch.empty((T, B), device=dev)
fns, lfns = ppo.bind(net.api), pl.bind(net.api)
h, s = net._handle, _stream(dev)
gae_args = ppo._gae_args(s, T, B, gamma, lam, rewards=rew, values=val, v_last=v_last, nonterminal=live, adv=adv_buf, ret=ret_buf)


def gae():
    net.api.check(fns['eb_gae'](C.byref(gae_args)))


def gae_torch():
    """examples/ppo_env_loop.py's loop, verbatim"""
    v_next = v_last
    adv = torch.empty((T, B), device=dev)
    run_adv = torch.zeros(B, device=dev)
    for t in range(T - 1, -1, -1):
        delta = rew[t] + gamma * v_next * live[t] - val[t]
        run_adv = delta + gamma * lam * live[t] * run_adv
        adv[t] = run_adv
        v_next = val[t]
    return adv, adv + val


gae(); torch.cuda.synchronize()
adv_all = adv_buf.view(n).clone()
adv_norm = torch.stack([adv_all.mean(), 1.0 / (adv_all.std() + 1e-8)])
adv_normed = (adv_all - adv_all.mean()) / (adv_all.std() + 1e-8)                      # what the example hands its minibatches
out = {k: torch.empty((n,) if k != 'g_logits' else (n, 4), device=dev) for k in ('logp', 'ratio', 'surr', 'ent', 'g_logits')}
sur_args = ppo._args(s, n, 0, 1.0, clip, ent_coef, 1.0 / n, obs=obs, actions=actions, logp_old=logp_old, adv=adv_all, adv_norm=adv_norm, **out)
logp_args = pl._args(s, n, 0, 1.0, obs=obs, actions=actions, logp=out['logp'])


def surrogate():
    net.api.check(fns['eb_ppo_surrogate'](h, C.byref(sur_args)))


def logp():
    net.api.check(lfns['eb_policy_logp'](h, C.byref(logp_args)))


def loss():
    l, _ = ppo.policy_loss(net, obs, actions, logp_old, adv_all, 1.0, clip, ent_coef, adv_norm)
    for q in net.parameters():
        q.grad = None
    l.backward()
    return l


def loss_torch():
    """examples/ppo_env_loop.py's minibatch, its policy part verbatim"""
    lp, logits = pl.log_prob(net, obs, actions, 1.0)
    ratio = (lp - logp_old).exp()
    policy_loss = -torch.min(ratio * adv_normed, ratio.clamp(1.0 - clip, 1.0 + clip) * adv_normed).mean()
    entropy = (logits[:, 2:] + 0.5 * math.log(2.0 * math.pi * math.e)).sum(1).mean()
    l = policy_loss - ent_coef * entropy
    for q in net.parameters():
        q.grad = None
    l.backward()
    return l


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


routes = {'gae': gae, 'gae_torch': gae_torch, 'loss': loss, 'loss_torch': loss_torch, 'surrogate': surrogate, 'logp': logp}
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='ppo', n=n, T=T, envs=B, net='%d -> 256 -> 256 -> 4, elu / linear, scale set, action_range 1' % obs_dim, iters=a.iters)
for k in routes:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
rec['gae_torch_over_gae'] = round(us['gae_torch'] / us['gae'], 3)
rec['loss_torch_over_loss'] = round(us['loss_torch'] / us['loss'], 3)
rec['surrogate_over_logp'] = round(us['surrogate'] / us['logp'], 3)
# the two sides compute the same things: GAE the same bits, the loss the same number up to float32 reductions
gae(); torch.cuda.synchronize()
ta, tr = gae_torch()
rec['gae_equals_torch'] = bool(torch.equal(ta, adv_buf) and torch.equal(tr, ret_buf))
l1, l2 = float(loss().detach()), float(loss_torch().detach())
rec['loss'], rec['loss_torch'] = l1, l2
g1 = [q.grad.clone() for q in net.parameters()]
loss()
rec['grad_rel_diff_max'] = max(float((q.grad - g).abs().max() / g.abs().max()) for q, g in zip(net.parameters(), g1))
surrogate(); torch.cuda.synchronize()
rec['clip_fraction'] = float(((out['ratio'] - 1.0).abs() > clip).float().mean())
if a.gae_envs:
    # eb_gae where its launch no longer counts: 3 arrays read and 2 written per (step, env), v_last besides
    Bl = a.gae_envs
    big = {k: torch.rand((T, Bl), device=dev) for k in ('rewards', 'values', 'nonterminal', 'adv', 'ret')}
    big_args = ppo._gae_args(s, T, Bl, gamma, lam, v_last=torch.rand((Bl,), device=dev), **big)
    big_gae = lambda: net.api.check(fns['eb_gae'](C.byref(big_args)))
    for _ in range(3): big_gae()
    torch.cuda.synchronize()
    tb = [window(big_gae) for _ in range(a.windows)]
    rec['gae_large_envs'], rec['gae_large_us'], rec['gae_large_us_windows'] = Bl, r(med(tb)), [r(v) for v in tb]
    rec['gae_large_gb_per_s'] = round((5 * T + 1) * Bl * 4 / med(tb) / 1e3, 1)
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
