"""ppo_env_loop.py — one PPO iteration on the batched `CrossroadEnd2end`: collect with the stochastic head, then optimise the clipped
surrogate through the log-probability of the STORED actions under the moving weights.

    out = sample_actions(policy, obs, action_range, seed=seed, counter=t)     # ONE launch (csrc/eb_policy_sample.hip)
    obs, reward, done, info = env.step(out['actions'])                        # ONE launch (csrc/eb_env_step.hip), finished envs reset
    ...
    logp_old = log_prob_actions(policy, obs_all, actions_all, action_range)   # ONE launch (csrc/eb_policy_logp.hip), no graph
    logp, logits = log_prob(policy, obs_mb, actions_mb, action_range)         # the same launch as an autograd node: both on the graph
    ratio = (logp - logp_old[idx]).exp()                                      # exactly 1.0 on the first pass: same entry, same weights
    loss = clipped surrogate - ent_coef * entropy(logits) + vf_coef * value loss
    loss.backward()                                                           # eb_policy_logp_vjp + ONE eb_mlp_backward per network

logp_old comes from eb_policy_logp, not from the sampler: the sampler's logp belongs to the unrounded pre-squash value, and atanh of
the rounded action differs from it (include/envbuild_policy_logp.h).  The value network is the reference's obj_v (one output, relu).
Generalised advantage estimation is a reverse loop over the steps in torch: it runs once per batch and is not the hot path.
Everything below the Python calls runs in libenvbuild_hip.so; there is no CPU path.
Run: python examples/ppo_env_loop.py [n_env] [steps]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                        # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402
from env_build_amd.policy_logp import log_prob, log_prob_actions    # noqa: E402
from env_build_amd.policy_sample import sample_actions              # noqa: E402


def run(n_env=4096, steps=32, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99, lam=0.95,
        clip=0.2, ent_coef=1e-3, vf_coef=0.5, lr=3e-4):
    """-> dict(policy_loss, value_loss, entropy: of the last minibatch; ratio_first: the first minibatch's ratio [rows] (numpy);
    policy_delta, value_delta: the largest change of a parameter; steps_per_s: of the collection)"""
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

    # ---- returns and advantages (GAE), once per batch ----
    obs_all, act_all = obs_buf.view(T * B, D), act_buf.view(T * B, 2)
    with torch.no_grad():
        v = value(obs_all)[:, 0].view(T, B)
        v_next = value(obs.t)[:, 0]
        adv = torch.empty((T, B), device=dev)
        run_adv = torch.zeros(B, device=dev)
        for t in range(T - 1, -1, -1):
            delta = rew_buf[t] + gamma * v_next * live_buf[t] - v[t]
            run_adv = delta + gamma * lam * live_buf[t] * run_adv
            adv[t] = run_adv
            v_next = v[t]
        ret_all = (adv + v).view(T * B)
        adv_all = adv.view(T * B)
        adv_all = (adv_all - adv_all.mean()) / (adv_all.std() + 1e-8)
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
            logp, logits = log_prob(policy, obs_all[idx], act_all[idx], action_range)
            ratio = (logp - logp_old[idx]).exp()
            if ratio_first is None:
                ratio_first = ratio.detach().cpu().numpy()
            a = adv_all[idx]
            policy_loss = -torch.min(ratio * a, ratio.clamp(1.0 - clip, 1.0 + clip) * a).mean()
            entropy = (logits[:, 2:] + 0.5 * math.log(2.0 * math.pi * math.e)).sum(1).mean()    # of the Gaussian before the squash
            value_loss = 0.5 * ((value(obs_all[idx])[:, 0] - ret_all[idx]) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            (policy_loss - ent_coef * entropy + vf_coef * value_loss).backward()
            opt.step()
            out = dict(policy_loss=float(policy_loss.detach()), value_loss=float(value_loss.detach()), entropy=float(entropy.detach()))
    n_pol = len(policy.parameters())
    delta = [float((p.detach() - b).abs().max()) for p, b in zip(params, before)]
    out.update(ratio_first=ratio_first, policy_delta=max(delta[:n_pol]), value_delta=max(delta[n_pol:]), steps_per_s=steps_per_s)
    return out


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    res = run(B, K)
    r = res.pop('ratio_first')
    print(dict(res, ratio_first_min=float(r.min()), ratio_first_max=float(r.max())))
