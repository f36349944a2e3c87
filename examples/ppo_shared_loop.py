"""ppo_shared_loop.py — ppo_scheduled_loop.py on ONE shared-trunk actor-critic network (env_build_amd.ac): obs -> 256 -> 256 -> 2 * act_dim + 1,
the policy's mean and log-std in the first 2 * act_dim columns and the value in the last.  A minibatch is one forward, one loss launch
(eb_ac_loss), one backward and Adam over one parameter set — 8 kernels where the two-network chain has 13 — and during collection the value
of every visited state falls out of the forward that samples its action (eb_ac_sample).  The learning-rate table and the KL stop are
ppo_scheduled_loop.py's, on the device.

    net = ac.make_net(obs_dim, 2, 256, 'elu', act_dim)
    col = ac.Collector(env, net, steps, action_range, seed=seed)
    upd = ac.PPOUpdate(net, rows, ..., lr_table=[...], target_kl=0.015)         # also a ctl.PPOUpdate
    loop = ctl.PPOEpochs(upd, col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()
    for every iteration:
        col.collect(); col.finish(gamma, lam); loop.replay(graph); loop.log()
    policy, value = ac.split(net)                                                # 2 * act_dim-wide and 1-wide MLPNets for inference

This is an option, not a recommendation: a shared trunk is a different model from two networks, and nothing here says it learns better.
There is no CPU path.
Run: python examples/ppo_shared_loop.py [n_env] [steps] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np                                                  # noqa: E402
import torch                                                        # noqa: E402
from env_build_amd import ac, ctl                                   # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402


def linear_table(iterations):
    """one factor per iteration, from 1 down to 0 at the last one"""
    return np.linspace(1.0, 0.0, iterations).astype(np.float32) if iterations > 1 else np.ones(1, np.float32)


def run(n_env=4096, steps=32, iterations=8, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99,
        lam=0.95, clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=3e-4, max_grad_norm=0.5, max_episode_steps=200, target_kl=0.015,
        kl_factor=1.5):
    """-> dict(logs: ctl.PPOEpochs.log() per iteration; table; limit; episodes: Collector.episodes() per iteration; deltas: per iteration the
    largest change of a parameter of the shared net; optimiser_steps and iterations_begun: the device's counts; mode and logits: the split
    policy's mode actions and logits on the env's last observations; shared: the shared net's outputs on the same rows)"""
    env = CrossroadEnd2end(task, n_env=n_env, auto_reset=True, copy_outputs=False, max_episode_steps=max_episode_steps)
    env.seed(seed)
    env.reset()
    env.reset()
    dev, D, T, B, A = env.device, env.obs_dim, steps, n_env, env.action_number
    scale = [0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num
    net = ac.make_net(D, 2, num_hidden_units, 'elu', A, device=dev, seed=seed)
    net.set_obs_scale(scale)

    col = ac.Collector(env, net, T, action_range, seed=seed)
    rows = T * B // minibatches
    table = linear_table(iterations)
    upd = ac.PPOUpdate(net, rows, action_range, clip, lr_table=table, target_kl=target_kl, kl_factor=kl_factor, max_slots=epochs * minibatches,
                       ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_grad_norm)
    loop = ctl.PPOEpochs(upd, col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()                                          # nothing runs; every replay reads the control block and the table
    logs, episodes, deltas = [], [], []
    for _ in range(iterations):
        before = net._flat.detach().clone()
        col.collect()
        col.finish(gamma, lam)
        loop.replay(graph)
        logs.append(loop.log())                                     # the host read of the update phase
        episodes.append(col.episodes())
        deltas.append(float((net._flat.detach() - before).abs().max()))
    # the trained net for the consumers of a 2 * act_dim-wide handle: Policy4Toyota.compute_mode's forward on the split policy
    policy, _value = ac.split(net)
    obs = env.obs.t.clone()
    mode = policy.mode(obs, action_range).numpy()
    logits = policy.call(obs).numpy()
    with torch.no_grad():
        shared = net.call(obs).cpu().numpy()
    return dict(logs=logs, episodes=episodes, deltas=deltas, table=table, limit=upd.control.limit, optimiser_steps=int(upd.adam.state.step),
                iterations_begun=upd.control.host()['iteration'], mode=mode, logits=logits, shared=shared)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    res = run(B, K, N)
    print('stop when the approximate KL of a minibatch is not <= %.4g' % res['limit'])
    for i, (log, ep, delta) in enumerate(zip(res['logs'], res['episodes'], res['deltas'])):
        steps_taken = int(log['applied'].sum())
        print('iteration %d: lr scale %.4f, stopped_at %d (%d of %d optimiser steps taken), %d episodes ended, return %.3f, largest '
              'parameter change %.3e' % (i, log['lr_scale'], log['stopped_at'], steps_taken, log['applied'].size, ep['episodes'],
                                         ep['return_mean'], delta))
    same = np.array_equal(res['logits'], res['shared'][:, :res['logits'].shape[1]])
    print(dict(optimiser_steps=res['optimiser_steps'], iterations_begun=res['iterations_begun'], split_policy_equals_the_shared_columns=same))
