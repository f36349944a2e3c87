"""ppo_fused_loop.py — the PPO iteration of ppo_env_loop.py with the update's arithmetic off torch: generalised advantage estimation in
ONE launch, and per minibatch the log-probability of the stored actions, the ratio, the clipped surrogate, the entropy bonus and the
cotangent of the logits in ONE launch with the policy network.

    adv, ret = gae(rew_buf, v, v_last, live_buf, gamma, lam)                  # ONE launch (csrc/eb_ppo.hip): ppo_env_loop.py's loop, bit for bit
    adv_norm = torch.stack([adv.mean(), 1 / (adv.std() + 1e-8)])              # two floats that stay on the device
    logp_old = log_prob_actions(policy, obs_all, actions_all, action_range)   # ONE launch (csrc/eb_policy_logp.hip), no graph
    loss, rows = policy_loss(policy, obs_mb, actions_mb, logp_old[idx], adv[idx], action_range, clip, ent_coef, adv_norm)
    (loss + vf_coef * value_loss).backward()                                  # the policy's part: ONE eb_mlp_backward, nothing else

rows['ratio'] is exactly 1.0 on the first pass: policy_loss calls the device function eb_policy_logp calls.  The advantages are
normalised in the kernel from adv_norm; the host never reads them.  The value network and its loss stay TrainableMLPNet + torch.
Everything below the Python calls runs in libenvbuild_hip.so; there is no CPU path.
Run: python examples/ppo_fused_loop.py [n_env] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                        # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402
from env_build_amd.policy_logp import log_prob_actions              # noqa: E402
from env_build_amd.policy_sample import sample_actions              # noqa: E402
from env_build_amd.ppo import gae, policy_loss                      # noqa: E402


def run(n_env=4096, steps=32, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99, lam=0.95,
        clip=0.2, ent_coef=1e-3, vf_coef=0.5, lr=3e-4, keep_buffers=False):
    """-> dict(policy_loss, value_loss, entropy, clip_fraction, approx_kl: of the last minibatch; ratio_first: the first minibatch's ratio
    [rows] (numpy); policy_delta, value_delta: the largest change of a parameter; steps_per_s: of the collection; with keep_buffers also
    buffers: the device tensors advantage estimation read and wrote (rewards, values, v_last, nonterminal, adv, ret))"""
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
        adv_all, ret_all = adv.t.view(T * B), ret.t.view(T * B)
        adv_norm = torch.stack([adv_all.mean(), 1.0 / (adv_all.std() + 1e-8)])
    logp_old = log_prob_actions(policy, obs_all, act_all, action_range)['logp'].t

    # ---- epochs x minibatches of the clipped surrogate ----
    params = policy.parameters() + value.parameters()
    before = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=lr)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    ratio_first, out = None, {}
    for _epoch in range(epochs):
        perm = torch.randperm(T * B, generator=gen).to(dev)
        for idx in perm.chunk(minibatches):
            loss, rows = policy_loss(policy, obs_all[idx], act_all[idx], logp_old[idx], adv_all[idx], action_range, clip, ent_coef, adv_norm)
            if ratio_first is None:
                ratio_first = rows['ratio'].cpu().numpy()
            value_loss = 0.5 * ((value(obs_all[idx])[:, 0] - ret_all[idx]) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            (loss + vf_coef * value_loss).backward()
            opt.step()
            out = dict(policy_loss=float(-rows['surr'].mean()), value_loss=float(value_loss.detach()), entropy=float(rows['ent'].mean()),
                       clip_fraction=float(((rows['ratio'] - 1.0).abs() > clip).float().mean()),
                       approx_kl=float((logp_old[idx] - rows['logp']).mean()))
    n_pol = len(policy.parameters())
    delta = [float((p.detach() - b).abs().max()) for p, b in zip(params, before)]
    out.update(ratio_first=ratio_first, policy_delta=max(delta[:n_pol]), value_delta=max(delta[n_pol:]), steps_per_s=steps_per_s)
    if keep_buffers:
        out['buffers'] = dict(rewards=rew_buf, values=v, v_last=v_last, nonterminal=live_buf, adv=adv.t, ret=ret.t)
    return out


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    res = run(B, K)
    r = res.pop('ratio_first')
    print(dict(res, ratio_first_min=float(r.min()), ratio_first_max=float(r.max())))
