"""ppo_scheduled_loop.py — ppo_collect_loop.py with the two controls every long PPO run turns on, both on the DEVICE so that the captured
update phase obeys them at every replay (env_build_amd.ctl): the learning rate annealed linearly to 0 over the run — a table of one factor
per iteration, read by eb_ctl_begin at the head of the graph — and the trust-region check — the optimiser steps of an iteration end at the
first minibatch whose approximate KL exceeds 1.5 * target_kl (eb_kl_stop before every eb_adam_step_ctl).

    upd = ctl.PPOUpdate(policy, value, rows, ..., lr_table=[1 - i / (iterations - 1) ...], target_kl=0.015)
    loop = ctl.PPOEpochs(upd, col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()                                                     # one linear graph, as before
    for every iteration:
        col.collect(); col.finish(gamma, lam)
        loop.replay(graph)                                                     # the next factor of the table; the stop cleared
        loop.log()                                                             # + lr_scale, applied, stopped_at

A captured graph cannot branch: after a stop the remaining minibatches still run their forward, backward and log.  The gain is the trust
region, not time.  There is no CPU path.
Run: python examples/ppo_scheduled_loop.py [n_env] [steps] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np                                                  # noqa: E402
import torch                                                        # noqa: E402
from env_build_amd import ctl                                       # noqa: E402
from env_build_amd.collect import Collector                         # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402


def linear_table(iterations):
    """one factor per iteration, from 1 down to 0 at the last one"""
    return np.linspace(1.0, 0.0, iterations).astype(np.float32) if iterations > 1 else np.ones(1, np.float32)


def run(n_env=4096, steps=32, iterations=8, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99,
        lam=0.95, clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=3e-4, max_grad_norm=0.5, max_episode_steps=200, target_kl=0.015,
        kl_factor=1.5):
    """-> dict(logs: ctl.PPOEpochs.log() per iteration — PPOEpochs' entries [epochs, minibatches], and lr_scale, applied, stopped_at;
    table: the factors; limit: kl_factor * target_kl; episodes: Collector.episodes() per iteration; deltas: per iteration the largest
    change of a (policy, value) parameter; optimiser_steps and iterations_begun: the device's counts)"""
    env = CrossroadEnd2end(task, n_env=n_env, auto_reset=True, copy_outputs=False, max_episode_steps=max_episode_steps)
    env.seed(seed)
    env.reset()
    env.reset()
    dev, D, T, B = env.device, env.obs_dim, steps, n_env
    scale = [0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num
    policy = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 4, output_activation='linear', name='policy', device=dev, seed=seed)
    value = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 1, output_activation='relu', name='obj_v', device=dev, seed=seed + 1)
    policy.set_obs_scale(scale)
    value.set_obs_scale(scale)

    col = Collector(env, policy, value, T, action_range, seed=seed)
    rows = T * B // minibatches
    table = linear_table(iterations)
    upd = ctl.PPOUpdate(policy, value, rows, action_range, clip, lr_table=table, target_kl=target_kl, kl_factor=kl_factor,
                        max_slots=epochs * minibatches, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr, max_grad_norm=max_grad_norm)
    loop = ctl.PPOEpochs(upd, col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()                                          # nothing runs; every replay reads the control block and the table
    logs, episodes, deltas = [], [], []
    for _ in range(iterations):
        before = [net._flat.detach().clone() for net in (policy, value)]
        col.collect()
        col.finish(gamma, lam)
        loop.replay(graph)
        logs.append(loop.log())                                     # the host read of the update phase
        episodes.append(col.episodes())
        deltas.append(tuple(float((net._flat.detach() - b).abs().max()) for net, b in zip((policy, value), before)))
    return dict(logs=logs, episodes=episodes, deltas=deltas, table=table, limit=upd.control.limit, optimiser_steps=int(upd.adam.state.step),
                iterations_begun=upd.control.host()['iteration'])


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    res = run(B, K, N)
    print('stop when the approximate KL of a minibatch is not <= %.4g' % res['limit'])
    for i, (log, ep, delta) in enumerate(zip(res['logs'], res['episodes'], res['deltas'])):
        steps_taken = int(log['applied'].sum())
        print('iteration %d: lr scale %.4f, stopped_at %d (%d of %d optimiser steps taken), %d episodes ended, return %.3f, largest '
              'parameter change %.3e / %.3e' % (i, log['lr_scale'], log['stopped_at'], steps_taken, log['applied'].size, ep['episodes'],
                                                ep['return_mean'], delta[0], delta[1]))
        for e in range(log['approx_kl'].shape[0]):
            print('  epoch %d  approx_kl %s   applied %s' % (e, ' '.join('%+.3e' % x for x in log['approx_kl'][e]),
                                                          ' '.join('%d' % x for x in log['applied'][e])))
    print(dict(optimiser_steps=res['optimiser_steps'], iterations_begun=res['iterations_begun']))
