"""ppo_captured_loop.py — the PPO iteration of ppo_fused_loop.py with the whole minibatch off torch: the surrogate, both backward passes,
the value loss, Adam with gradient clipping and the weight refresh are ONE captured chain of 13 library kernels
(env_build_amd.train.PPOUpdate), replayed once per minibatch.

    upd = PPOUpdate(policy, value, rows, action_range, clip, ent_coef, vf_coef, clip_v, lr=lr, max_grad_norm=0.5)
    graph = upd.capture()                                                      # nothing runs; the optimiser state lives on the device
    perm = torch.randperm(T * B, device=dev)                                   # per epoch, on the device
    torch.index_select(obs_all, 0, idx, out=upd.mb.obs) ...                    # the gather: the caller's, outside the chain
    upd.replay(graph)                                                          # one minibatch; the next replay takes the next Adam step

Collection, advantage estimation and logp_old are ppo_fused_loop.py's.  Logging is read once per epoch from upd.rows.*, not per
minibatch: a replay makes no host read.  Everything below the Python calls runs in libenvbuild_hip.so and libenvbuild_train.so; there
is no CPU path.
Run: python examples/ppo_captured_loop.py [n_env] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                        # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402
from env_build_amd.policy_logp import log_prob_actions              # noqa: E402
from env_build_amd.policy_sample import sample_actions              # noqa: E402
from env_build_amd.ppo import gae                                   # noqa: E402
from env_build_amd.train import PPOUpdate                           # noqa: E402


def run(n_env=4096, steps=32, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99, lam=0.95,
        clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=3e-4, max_grad_norm=0.5):
    """-> dict(policy_loss, value_loss, entropy, clip_fraction, approx_kl: of the last minibatch of the last epoch; grad_norm: of the last
    step; optimiser_steps: the device's count; ratio_first: the first minibatch's ratio [rows] (numpy); policy_delta, value_delta: the
    largest change of a parameter; steps_per_s: of the collection)"""
    env = CrossroadEnd2end(task, n_env=n_env, auto_reset=True, copy_outputs=False)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    dev, D, T, B = env.device, env.obs_dim, steps, n_env
    scale = [0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num
    policy = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 4, output_activation='linear', name='policy', device=dev, seed=seed)
    value = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 1, output_activation='relu', name='obj_v', device=dev, seed=seed + 1)
    policy.set_obs_scale(scale)
    value.set_obs_scale(scale)

    # ---- collect T steps x B envs: two launches per step, everything stays on the device ----
    obs_buf = torch.empty((T, B, D), device=dev)
    act_buf = torch.empty((T, B, 2), device=dev)
    rew_buf = torch.empty((T, B), device=dev)
    live_buf = torch.empty((T, B), device=dev)                      # 0 where the step ended its episode
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(T):
        obs_buf[t].copy_(obs.t)                                     # copy_outputs=False: the env reuses its observation buffer
        out = sample_actions(policy, obs_buf[t], action_range, seed=seed, counter=t, want=())
        act_buf[t].copy_(out['actions'].t)
        obs, reward, _done, _info = env.step(out['actions'])
        rew_buf[t].copy_(reward.t)
        live_buf[t].copy_(env.done_code == 0)
    torch.cuda.synchronize()
    steps_per_s = B * T / (time.perf_counter() - t0)

    # ---- returns and advantages (GAE): one launch; the normalisation is two floats on the device ----
    obs_all, act_all = obs_buf.view(T * B, D), act_buf.view(T * B, 2)
    with torch.no_grad():
        v = value(obs_all)[:, 0].view(T, B).contiguous()
        v_last = value(obs.t)[:, 0].contiguous()
        adv, ret = gae(rew_buf, v, v_last, live_buf, gamma, lam)
        adv_all, ret_all, v_all = adv.t.view(T * B), ret.t.view(T * B), v.view(T * B)
        adv_norm = torch.stack([adv_all.mean(), 1.0 / (adv_all.std() + 1e-8)])
    logp_old = log_prob_actions(policy, obs_all, act_all, action_range)['logp'].t

    # ---- epochs x minibatches: one captured chain, replayed ----
    rows = T * B // minibatches
    before = [p.detach().clone() for p in policy.parameters() + value.parameters()]
    upd = PPOUpdate(policy, value, rows, action_range, clip, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr,
                    max_grad_norm=max_grad_norm)
    upd.mb.adv_norm.copy_(adv_norm)
    graph = upd.capture()
    torch.manual_seed(seed)
    sources = ((obs_all, upd.mb.obs), (act_all, upd.mb.actions), (logp_old, upd.mb.logp_old), (adv_all, upd.mb.adv), (ret_all, upd.mb.ret),
               (v_all, upd.mb.v_old))
    ratio_first, out = None, {}
    for _epoch in range(epochs):
        perm = torch.randperm(T * B, device=dev)
        for k in range(minibatches):
            idx = perm[k * rows:(k + 1) * rows]
            for src, dst in sources:                                # the gather: the caller's job, outside the chain
                torch.index_select(src, 0, idx, out=dst)
            upd.replay(graph)
            if ratio_first is None:
                ratio_first = upd.rows.ratio.cpu().numpy()
        r = upd.rows                                                # once per epoch: the last minibatch's rows
        out = dict(policy_loss=float(-r.surr.mean()), value_loss=float(r.vloss.mean()), entropy=float(r.ent.mean()),
                   clip_fraction=float(((r.ratio - 1.0).abs() > clip).float().mean()), approx_kl=float((upd.mb.logp_old - r.logp).mean()),
                   grad_norm=float(upd.adam.state.gnorm))
    n_pol = len(policy.parameters())
    delta = [float((p.detach() - b).abs().max()) for p, b in zip(policy.parameters() + value.parameters(), before)]
    out.update(ratio_first=ratio_first, policy_delta=max(delta[:n_pol]), value_delta=max(delta[n_pol:]), steps_per_s=steps_per_s,
               optimiser_steps=int(upd.adam.state.step))
    return out


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    res = run(B, K)
    r = res.pop('ratio_first')
    print(dict(res, ratio_first_min=float(r.min()), ratio_first_max=float(r.max())))
