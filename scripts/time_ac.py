#!/usr/bin/env python3
"""Profiling aid: the shared-trunk actor-critic route (env_build_amd.ac: ONE network obs_dim -> 256 -> 256 -> 5) against the two-network
route (obs_dim -> 256 -> 256 -> 4 | 1) in ONE process on cuda:0, HIP events on the launch stream, alternating windows, median with spread
(the discipline of scripts/time_ctl.py).  Three routes, each pair on the same data:

  (minibatch)   train.PPOUpdate.replay (13 kernels)                 against ac.PPOUpdate.replay (8 kernels), `rows` rows
  (epochs)      epoch.PPOEpochs.replay, epochs x minibatches        against the same driver over ac.PPOUpdate
  (collect)     collect.Collector.collect() + finish()              against ac.Collector's, n_env envs x steps steps — with the env, so only at
                                                                    the env's own width (41 for `left`); other widths time the launches of a
                                                                    step and of the head without an env

and the two new entries on their own, per call, next to the existing entries they stand for: (ac_loss) eb_ac_loss against (surrogate +
value_loss) eb_ppo_surrogate_from_logits + eb_value_loss, (ac_sample) eb_ac_sample against (sample) eb_policy_sample_from_logits.

Timing is recorded, not asserted.  Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_ac.py [--rows 4096] [--obs-dim 41] [--epochs 4] [--minibatches 4] [--n-env 4096] [--steps 32] [--iters 5]
                              [--part-iters 100] [--windows 5] [--out FILE] [--append]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd import _capi, ac, collect, epoch, ppo, train
from env_build_amd import policy_logp as pl
from env_build_amd import policy_sample as ps
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=4096); ap.add_argument('--obs-dim', type=int, default=41)
ap.add_argument('--epochs', type=int, default=4); ap.add_argument('--minibatches', type=int, default=4)
ap.add_argument('--n-env', type=int, default=4096); ap.add_argument('--steps', type=int, default=32)
ap.add_argument('--iters', type=int, default=5); ap.add_argument('--part-iters', type=int, default=100)
ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r28_ac_timing.txt'))
ap.add_argument('--append', action='store_true', help='add the record to --out (a second shape) instead of replacing the file')
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
r = lambda v: round(v, 1)
head = '# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)
print(head, flush=True)

rows, D, E, M, B, T = a.rows, a.obs_dim, a.epochs, a.minibatches, a.n_env, a.steps
N = M * rows
clip, ent_coef, vf_coef, clip_v, lr, max_norm = 0.2, 1e-3, 0.5, 0.2, 1e-5, 0.5     # a small lr: hundreds of steps on one set of data
rng = np.random.default_rng(0)
gpu = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
with_env = D == 41
scale = rng.uniform(0.02, 0.2, D).astype(np.float32)               # of the update routes' networks: synthetic observations N(0, 100)
env_scale = np.array([0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * 8, np.float32)


def two_nets(sc=scale):
    policy = TrainableMLPNet(D, 2, 256, 'elu', 4, output_activation='linear', device=dev, seed=0)
    value = TrainableMLPNet(D, 2, 256, 'elu', 1, output_activation='relu', device=dev, seed=1)
    policy.set_obs_scale(sc); value.set_obs_scale(sc)
    return policy, value


def one_net(sc=scale):
    net = ac.make_net(D, 2, 256, 'elu', 2, device=dev, seed=0)
    net.set_obs_scale(sc)
    return net


kw = dict(ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_norm)
obs = gpu(rng.standard_normal((N, D)) * 10)


def data_for(policy, value_of):
    actions = ps.sample_actions(policy, obs, 1.0, seed=1, want=())['actions'].t.clone()
    logp_old = (pl.log_prob_actions(policy, obs, actions, 1.0)['logp'].t + gpu(rng.uniform(-0.4, 0.4, N))).contiguous()
    v_old = value_of(obs).clone()
    return dict(obs=obs, actions=actions.contiguous(), logp_old=logp_old, adv=gpu(rng.standard_normal(N)), ret=v_old + gpu(rng.uniform(-0.6, 0.6, N)),
                v_old=v_old)


def fill(upd, data):
    for k in ('obs', 'actions', 'logp_old', 'adv', 'ret', 'v_old'):
        getattr(upd.mb, k).copy_(data[k][:rows])


# ---- the two-network route ----
pol_m, val_m = two_nets(); pol_e, val_e = two_nets()
with torch.no_grad():
    data_two = data_for(pol_m, lambda x: val_m(x)[:, 0])
upd_two = train.PPOUpdate(pol_m, val_m, rows, 1.0, clip, **kw)
fill(upd_two, data_two)
g_upd_two = upd_two.capture()
loop_two = epoch.PPOEpochs(train.PPOUpdate(pol_e, val_e, rows, 1.0, clip, **kw), data_two, E, M, seed=0)
g_loop_two = loop_two.capture()
# ---- the shared route ----
net_m, net_e = one_net(), one_net()
split_policy, split_value = ac.split(net_m)
data_one = data_for(split_policy, lambda x: split_value.call(x).t[:, 0])
upd_one = ac.PPOUpdate(net_m, rows, 1.0, clip, **kw)
fill(upd_one, data_one)
g_upd_one = upd_one.capture()
loop_one = epoch.PPOEpochs(ac.PPOUpdate(net_e, rows, 1.0, clip, **kw), data_one, E, M, seed=0)
g_loop_one = loop_one.capture()
routes = {'minibatch_two': lambda: upd_two.replay(g_upd_two), 'minibatch_shared': lambda: upd_one.replay(g_upd_one),
          'epochs_two': lambda: loop_two.replay(g_loop_two), 'epochs_shared': lambda: loop_one.replay(g_loop_one)}

# ---- collection: with the env at its own width, the launches alone otherwise ----
pol_c, val_c = two_nets(env_scale if with_env else scale); net_c = one_net(env_scale if with_env else scale)   # the env's own observations
if with_env:
    from env_build_amd.endtoend import CrossroadEnd2end

    def env():
        e = CrossroadEnd2end('left', n_env=B, auto_reset=True, copy_outputs=False, max_episode_steps=max(T, 200))
        e.seed(0); e.reset(); e.reset()
        return e
    col_two, col_one = collect.Collector(env(), pol_c, val_c, T, 1.0, seed=0), ac.Collector(env(), net_c, T, 1.0, seed=0)

    def collect_two(): col_two.collect(); col_two.finish(0.99, 0.95)
    def collect_one(): col_one.collect(); col_one.finish(0.99, 0.95)
else:
    raw = pol_c._stream()
    api, aca = pol_c.api, ac.ac_api()
    sample_fn = ps.bind(api)['eb_policy_sample']
    step_obs, all_obs = gpu(rng.standard_normal((B, D)) * 10), gpu(rng.standard_normal(((T + 1) * B, D)) * 10)
    act, logit, y, vals, all_vals = (torch.zeros(s, device=dev) for s in ((B, 2), (B, 4), (B, 5), (B,), ((T + 1) * B,)))
    sm = ac.EbAcSampleArgs(n=B, act_dim=2, y=y.data_ptr(), seed=0, counter=0, action_range=1.0, actions=act.data_ptr(), logits_out=logit.data_ptr(),
                           values=vals.data_ptr(), stream=raw)
    sp = ac.EbAcSampleArgs(n=B, act_dim=2, y=y.data_ptr(), action_range=1.0, values=vals.data_ptr(), stream=raw)
    hp, hv, hn = pol_c._handle, val_c._handle, net_c._handle

    def collect_two():                                            # T sampling launches, the value forward over (T + 1) * B rows and over B rows
        for t in range(T):
            api.check(sample_fn(hp, B, step_obs.data_ptr(), None, None, 0, t, 1.0, act.data_ptr(), None, logit.data_ptr(), None, raw))
        api.mlp_forward(hv, (T + 1) * B, all_obs.data_ptr(), all_vals.data_ptr(), raw)
        api.mlp_forward(hv, B, step_obs.data_ptr(), vals.data_ptr(), raw)

    def collect_one():                                            # T x (forward, sample), two (forward, split) over B rows
        for t in range(T):
            api.mlp_forward(hn, B, step_obs.data_ptr(), y.data_ptr(), raw)
            sm.counter = t
            aca.check(aca.sample(C.byref(sm)))
        for _ in range(2):
            api.mlp_forward(hn, B, step_obs.data_ptr(), y.data_ptr(), raw)
            aca.check(aca.sample(C.byref(sp)))
routes.update(collect_two=collect_two, collect_shared=collect_one)

# ---- the entries alone, on one minibatch's rows ----
hip, tapi, acapi = _capi.hip_api(), train.train_api(), ac.ac_api()
raw = pol_m._stream()
mb, out = upd_one.mb, upd_one.rows
y_rows = upd_one.y
dense, g_logits, g_vals = torch.zeros((rows, 4), device=dev), torch.zeros((rows, 4), device=dev), torch.zeros((rows, 5), device=dev)
upd_one.replay(g_upd_one)                                         # y holds one forward's outputs
dense.copy_(y_rows[:, :4])
torch.cuda.synchronize()
loss_args = ac.EbAcLossArgs.from_buffer_copy(upd_one._ppo_args)
loss_args.stream = raw
sur_args = ppo._args(raw, rows, 4, 1.0, clip, ent_coef, 1.0 / rows, logits=dense, actions=mb.actions, logp_old=mb.logp_old, adv=mb.adv,
                     adv_norm=mb.adv_norm, logp=out.logp, ratio=out.ratio, surr=out.surr, ent=out.ent, g_logits=g_logits)
vl_args = train.EbValueLossArgs(n=rows, stride=5, values=y_rows.data_ptr() + 16, ret=mb.ret.data_ptr(), v_old=mb.v_old.data_ptr(), clip_v=clip_v,
                                scale=vf_coef / rows, loss=out.vloss.data_ptr(), g_values=g_vals.data_ptr() + 16, stream=raw)
surrogate_fn, sample_logits_fn = ppo.bind(hip)['eb_ppo_surrogate_from_logits'], ps.bind(hip)['eb_policy_sample_from_logits']
p_act, p_logit, p_val = torch.zeros((rows, 2), device=dev), torch.zeros((rows, 4), device=dev), torch.zeros((rows,), device=dev)
smp_args = ac.EbAcSampleArgs(n=rows, act_dim=2, y=y_rows.data_ptr(), seed=0, counter=0, action_range=1.0, actions=p_act.data_ptr(),
                             logits_out=p_logit.data_ptr(), values=p_val.data_ptr(), stream=raw)


def ac_loss(): acapi.check(acapi.loss(C.byref(loss_args)))
def surrogate_and_value_loss():
    hip.check(surrogate_fn(C.byref(sur_args))); tapi.check(tapi.value_loss(C.byref(vl_args)))
def ac_sample(): acapi.check(acapi.sample(C.byref(smp_args)))
def sample(): hip.check(sample_logits_fn(rows, 4, dense.data_ptr(), None, None, 0, 0, 1.0, p_act.data_ptr(), None, None, raw))


parts = {'ac_loss': ac_loss, 'surrogate_and_value_loss': surrogate_and_value_loss, 'ac_sample': ac_sample, 'sample': sample}


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for fn in list(routes.values()) + list(parts.values()):
    for _ in range(2): fn()
torch.cuda.synchronize()
times = {k: [] for k in list(routes) + list(parts)}
for _ in range(a.windows):
    for k, fn in routes.items():
        times[k].append(window(fn, a.part_iters if k.startswith('minibatch') else a.iters))
    for k, fn in parts.items():
        times[k].append(window(fn, a.part_iters))
us = {k: med(v) for k, v in times.items()}
rec = dict(what='ac', rows=rows, N=N, epochs=E, minibatches=M, n_env=B, steps=T, obs_dim=D, collect_with_env=with_env, iters=a.iters,
           part_iters=a.part_iters, nets='two: %d -> 256 -> 256 -> 4 | 1, elu / linear | relu; shared: %d -> 256 -> 256 -> 5, elu / linear' % (D, D),
           kernels={'minibatch_two': 13, 'minibatch_shared': 8, 'epochs_two': 3 + 15 * E * M, 'epochs_shared': 3 + 10 * E * M},
           unit='us per minibatch / per update phase / per collection + head / per call (the parts)')
for k in times:
    rec[k + '_us'] = r(us[k]); rec[k + '_us_windows'] = [r(v) for v in times[k]]; rec[k + '_spread_us'] = r(max(times[k]) - min(times[k]))
for k in ('minibatch', 'epochs', 'collect'):
    rec[k + '_two_over_shared'] = round(us[k + '_two'] / us[k + '_shared'], 3)
    rec[k + '_gain_beyond_spread'] = bool(us[k + '_two'] - us[k + '_shared'] > max(rec[k + '_two_spread_us'], rec[k + '_shared_spread_us']))
torch.cuda.synchronize()
rec['finite'] = bool(all(torch.isfinite(n._flat).all() for n in (pol_m, val_m, pol_e, val_e, net_m, net_e)))
line = json.dumps(rec)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'a' if a.append else 'w') as fh:
    fh.write(('' if a.append else head + '\n') + line + '\n')
