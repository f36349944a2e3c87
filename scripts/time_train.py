#!/usr/bin/env python3
"""Profiling aid: one PPO minibatch (policy and value network) at n x (obs_dim -> 256 -> 256 -> 4 | 1), elu hidden, linear / relu out,
scale set, action_range 1, in ONE process on cuda:0, HIP events on the launch stream, alternating windows (the discipline of
scripts/time_ppo.py).  The minibatch is fixed: the gather that fills it is outside every route.  Four routes, each on its own pair of
networks made from the same weights:

  (a) body            examples/ppo_fused_loop.py's minibatch body: policy_loss, the torch value loss, zero_grad, backward,
                      torch.optim.Adam (default) step
  (b) body_fused      the same with torch.optim.Adam(fused=True, capturable=True) and clip_grad_norm_ in front
  (c) step            PPOUpdate.step(), eager
  (d) replay          PPOUpdate.replay() of one PPOUpdate.capture()

and two parts on their own: (adam / adam_torch) eb_adam_step + 2 x eb_mlp_set_params_device against (b)'s optimiser part —
clip_grad_norm_, the fused capturable step and the two uploads its next forward makes —, and (vloss / vloss_torch) eb_value_loss against
the torch expression of the clipped value loss, forward + backward to the values.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_train.py [--n 65536] [--obs-dim 137] [--iters 100] [--windows 5] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd import ppo, train
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=65536); ap.add_argument('--obs-dim', type=int, default=137)
ap.add_argument('--iters', type=int, default=100); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r24_train_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

n, obs_dim = a.n, a.obs_dim
clip, ent_coef, vf_coef, clip_v, lr, max_norm = 0.2, 1e-3, 0.5, 0.2, 1e-5, 0.5     # a small lr: hundreds of steps on one minibatch
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
scale = rng.uniform(0.02, 0.2, obs_dim).astype(np.float32)


def nets():
    policy = TrainableMLPNet(obs_dim, 2, 256, 'elu', 4, output_activation='linear', device=dev, seed=0)
    value = TrainableMLPNet(obs_dim, 2, 256, 'elu', 1, output_activation='relu', device=dev, seed=1)
    policy.set_obs_scale(scale); value.set_obs_scale(scale)
    return policy, value


pol_a, val_a = nets(); pol_b, val_b = nets(); pol_c, val_c = nets(); pol_d, val_d = nets()
obs = gpu(rng.standard_normal((n, obs_dim)) * 10)
actions = ps.sample_actions(pol_a, obs, 1.0, seed=1, want=())['actions'].t.clone()
logp_old = pl.log_prob_actions(pol_a, obs, actions, 1.0)['logp'].t + gpu(rng.uniform(-0.4, 0.4, n))
adv = gpu(rng.standard_normal(n))
adv_norm = torch.stack([adv.mean(), 1.0 / (adv.std() + 1e-8)])
with torch.no_grad():
    v_old = val_a(obs)[:, 0].clone()
ret = v_old + gpu(rng.uniform(-0.6, 0.6, n))


def body(policy, value, opt, clipped):
    def run():
        loss, _rows = ppo.policy_loss(policy, obs, actions, logp_old, adv, 1.0, clip, ent_coef, adv_norm)
        v = value(obs)[:, 0]
        value_loss = (0.5 * torch.max((v - ret) ** 2, (v_old + (v - v_old).clamp(-clip_v, clip_v) - ret) ** 2)).mean()
        opt.zero_grad(set_to_none=True)
        (loss + vf_coef * value_loss).backward()
        if clipped:
            torch.nn.utils.clip_grad_norm_(opt.param_groups[0]['params'], max_norm)
        opt.step()
    return run


opt_a = torch.optim.Adam(pol_a.parameters() + val_a.parameters(), lr=lr)
opt_b = torch.optim.Adam(pol_b.parameters() + val_b.parameters(), lr=lr, fused=True, capturable=True)
upd_c = train.PPOUpdate(pol_c, val_c, n, 1.0, clip, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_norm)
upd_d = train.PPOUpdate(pol_d, val_d, n, 1.0, clip, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_norm)
for upd in (upd_c, upd_d):
    for dst, src in ((upd.mb.obs, obs), (upd.mb.actions, actions), (upd.mb.logp_old, logp_old), (upd.mb.adv, adv), (upd.mb.ret, ret),
                     (upd.mb.v_old, v_old), (upd.mb.adv_norm, adv_norm)):
        dst.copy_(src)
graph = upd_d.capture()

# the optimiser alone: gradients as (b) left them / as (c) left them
params_b = pol_b.parameters() + val_b.parameters()


def adam_torch():
    torch.nn.utils.clip_grad_norm_(params_b, max_norm)
    opt_b.step()
    pol_b._sync(); val_b._sync()


def adam():
    upd_c.adam.issue()
    upd_c.adam.bump()
    for net in (pol_c, val_c):
        net.api.mlp_set_params_device(net._h, net._flat.data_ptr(), net._stream())
        net._uploaded = net._flat._version


vals = val_a(obs).detach().clone()
vl_loss, vl_g = torch.empty((n,), device=dev), torch.empty((n, 1), device=dev)
vl_args = train.EbValueLossArgs(n=n, stride=1, values=vals.data_ptr(), ret=ret.data_ptr(), v_old=v_old.data_ptr(), clip_v=clip_v,
                                scale=vf_coef / n, loss=vl_loss.data_ptr(), g_values=vl_g.data_ptr(), stream=upd_c.policy._stream())
tapi = train.train_api()


def vloss():
    tapi.check(tapi.value_loss(C.byref(vl_args)))


def vloss_torch():
    v = vals[:, 0].detach().requires_grad_(True)
    value_loss = (0.5 * torch.max((v - ret) ** 2, (v_old + (v - v_old).clamp(-clip_v, clip_v) - ret) ** 2)).mean()
    (vf_coef * value_loss).backward()
    return v.grad


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


routes = {'body': body(pol_a, val_a, opt_a, False), 'body_fused': body(pol_b, val_b, opt_b, True), 'step': upd_c.step, 'replay': lambda: upd_d.replay(graph),
          'adam': adam, 'adam_torch': adam_torch, 'vloss': vloss, 'vloss_torch': vloss_torch}
for fn in routes.values():
    for _ in range(3): fn()
torch.cuda.synchronize()
times = {k: [] for k in routes}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='train', n=n, net='%d -> 256 -> 256 -> 4 | 1, elu / linear | relu, scale set, action_range 1' % obs_dim, iters=a.iters,
           params=int(pol_a._flat.numel() + val_a._flat.numel()))
for k in routes:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
rec['body_over_step'] = round(us['body'] / us['step'], 3)
rec['body_over_replay'] = round(us['body'] / us['replay'], 3)
rec['body_fused_over_replay'] = round(us['body_fused'] / us['replay'], 3)
rec['adam_torch_over_adam'] = round(us['adam_torch'] / us['adam'], 3)
rec['vloss_torch_over_vloss'] = round(us['vloss_torch'] / us['vloss'], 3)
# the routes compute the same thing: eager and captured the same bits (same number of steps each), the value loss gradient the torch one
torch.cuda.synchronize()
rec['steps_c'], rec['steps_d'] = int(upd_c.adam.state.step), int(upd_d.adam.state.step)
vloss(); torch.cuda.synchronize()
g_t = vloss_torch()
rec['vloss_grad_rel_diff_max'] = float((vl_g[:, 0] - g_t).abs().max() / g_t.abs().max())
rec['finite'] = bool(all(torch.isfinite(net._flat).all() for net in (pol_a, val_a, pol_b, val_b, pol_c, val_c, pol_d, val_d)))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
