"""ppo_epoch_loop.py — the PPO iteration of ppo_captured_loop.py with the WHOLE update phase as one captured chain, replayed once per
iteration (env_build_amd.epoch.PPOEpochs): the advantage statistics, and for every epoch and minibatch the keyed shuffle's gather of
all six tensors in one launch, the 13 kernels of train.PPOUpdate and the logging sums — no torch kernel, no host read and no Python loop
over minibatches between the first launch and the last.

    upd = PPOUpdate(policy, value, rows, action_range, clip, ent_coef, vf_coef, clip_v, lr=lr, max_grad_norm=0.5)
    loop = PPOEpochs(upd, dict(obs=..., actions=..., logp_old=..., adv=..., ret=..., v_old=...), epochs, minibatches, seed=seed)
    graph = loop.capture()                                                     # nothing runs; 3 + 15 * epochs * minibatches kernels
    loop.replay(graph)                                                         # one iteration's update phase
    log = loop.log()                                                           # one device-to-host copy: arrays [epochs, minibatches]

The permutation of an epoch is never in memory: minibatch k of epoch e takes the rows index(key(seed, counter + e), T * B, k * rows + r),
and the counter lives on the device, so the next replay shuffles anew.  Collection, advantage estimation and logp_old are
ppo_captured_loop.py's.  Everything below the Python calls runs in libenvbuild_hip.so, libenvbuild_train.so and libenvbuild_epoch.so;
there is no CPU path.
Run: python examples/ppo_epoch_loop.py [n_env] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                        # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.epoch import PPOEpochs                           # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402
from env_build_amd.policy_logp import log_prob_actions              # noqa: E402
from env_build_amd.policy_sample import sample_actions              # noqa: E402
from env_build_amd.ppo import gae                                   # noqa: E402
from env_build_amd.train import PPOUpdate                           # noqa: E402


def run(n_env=4096, steps=32, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99, lam=0.95,
        clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=3e-4, max_grad_norm=0.5):
    """-> dict(log: PPOEpochs.log(), every entry [epochs, minibatches]; grad_norm: of the last step; optimiser_steps and counter: the
    device's counts; policy_delta, value_delta: the largest change of a parameter; steps_per_s: of the collection)"""
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

    # ---- returns and advantages (GAE): one launch; the normalisation is the update chain's first two kernels ----
    obs_all, act_all = obs_buf.view(T * B, D), act_buf.view(T * B, 2)
    with torch.no_grad():
        v = value(obs_all)[:, 0].view(T, B).contiguous()
        v_last = value(obs.t)[:, 0].contiguous()
        adv, ret = gae(rew_buf, v, v_last, live_buf, gamma, lam)
        adv_all, ret_all, v_all = adv.t.view(T * B), ret.t.view(T * B), v.view(T * B)
    logp_old = log_prob_actions(policy, obs_all, act_all, action_range)['logp'].t

    # ---- epochs x minibatches: ONE captured chain, replayed once ----
    rows = T * B // minibatches
    before = [p.detach().clone() for p in policy.parameters() + value.parameters()]
    upd = PPOUpdate(policy, value, rows, action_range, clip, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr,
                    max_grad_norm=max_grad_norm)
    data = dict(obs=obs_all, actions=act_all, logp_old=logp_old.contiguous(), adv=adv_all.contiguous(), ret=ret_all.contiguous(),
                v_old=v_all.contiguous())
    loop = PPOEpochs(upd, data, epochs, minibatches, seed=seed)
    graph = loop.capture()
    loop.replay(graph)                                              # a training run refills `data` and replays again, every iteration
    log = loop.log()                                                # the one host read of the update phase
    n_pol = len(policy.parameters())
    delta = [float((p.detach() - b).abs().max()) for p, b in zip(policy.parameters() + value.parameters(), before)]
    return dict(log=log, grad_norm=float(upd.adam.state.gnorm), optimiser_steps=int(upd.adam.state.step), counter=int(loop.counter),
                policy_delta=max(delta[:n_pol]), value_delta=max(delta[n_pol:]), steps_per_s=steps_per_s)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    res = run(B, K)
    log = res.pop('log')
    print('epoch  approx_kl per minibatch' + ' ' * 30 + 'clip_fraction per minibatch')
    for e in range(log['approx_kl'].shape[0]):
        print('%5d  %s    %s' % (e, ' '.join('%+.3e' % x for x in log['approx_kl'][e]), ' '.join('%.4f' % x for x in log['clip_fraction'][e])))
    print(dict(res, policy_loss_last=float(log['policy_loss'][-1, -1]), value_loss_last=float(log['value_loss'][-1, -1]),
               entropy_last=float(log['entropy'][-1, -1]), max_ratio_dev_first=float(log['max_ratio_dev'][0, 0])))
