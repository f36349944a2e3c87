"""ppo_normalized_loop.py — ppo_collect_loop.py with the reference's default preprocessor: observations and rewards are normalised by RUNNING
statistics that live on the device (env_build_amd.norm.Collector, include/envbuild_norm.h) instead of a hand-tuned obs_scale vector and raw
rewards.  Per collected step, after eb_policy_sample, the env step and eb_collect_record: eb_norm_update (two launches: the batch sums and
the merge, observations and discounted returns together) and eb_norm_apply (one launch: the next observation, the final observations of
truncated episodes and the reward) — no torch operation, no allocation, no host read.

    col = norm.Collector(env, policy, value, steps, action_range, seed=seed, gamma=gamma)   # every buffer and both states, once
    loop = PPOEpochs(PPOUpdate(policy, value, rows, ...), col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()
    for every iteration:
        col.collect(); col.finish(gamma, lam); loop.replay(graph); loop.log(); col.episodes()

The networks see normalised observations and carry no obs_scale.  The episode log reports RAW returns.  Each iteration prints the
observation state's count and the largest |mean_f| and den_f.
Run: python examples/ppo_normalized_loop.py [n_env] [steps] [iterations]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                        # noqa: E402
from env_build_amd.norm import Collector                            # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.epoch import PPOEpochs                           # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402
from env_build_amd.train import PPOUpdate                           # noqa: E402


def run(n_env=4096, steps=32, iterations=4, epochs=4, minibatches=4, task='left', seed=0, num_hidden_units=256, action_range=1.0, gamma=0.99,
        lam=0.95, clip=0.2, ent_coef=1e-3, vf_coef=0.5, clip_v=0.2, lr=3e-4, max_grad_norm=0.5, max_episode_steps=200):
    """-> dict(logs: PPOEpochs.log() per iteration, every entry [epochs, minibatches]; episodes: Collector.episodes() per iteration;
    norm: per iteration, dict(count, ret_count, mean_abs_max, den_max, ret_den) of the two states; grad_norm: of the last step; optimiser_steps and counter: the device's counts; policy_delta, value_delta: the largest change of a
    parameter; steps_per_s: of collection + head over all iterations)"""
    env = CrossroadEnd2end(task, n_env=n_env, auto_reset=True, copy_outputs=False, max_episode_steps=max_episode_steps)
    env.seed(seed)
    env.reset()
    env.reset()
    dev, D, T, B = env.device, env.obs_dim, steps, n_env
    policy = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 4, output_activation='linear', name='policy', device=dev, seed=seed)
    value = TrainableMLPNet(D, 2, num_hidden_units, 'elu', 1, output_activation='relu', name='obj_v', device=dev, seed=seed + 1)

    col = Collector(env, policy, value, T, action_range, seed=seed, gamma=gamma)
    rows = T * B // minibatches
    before = [p.detach().clone() for p in policy.parameters() + value.parameters()]
    upd = PPOUpdate(policy, value, rows, action_range, clip, ent_coef=ent_coef, vf_coef=vf_coef, clip_v=clip_v, lr=lr,
                    max_grad_norm=max_grad_norm)
    loop = PPOEpochs(upd, col.data, epochs, minibatches, seed=seed)
    graph = loop.capture()                                          # nothing runs; every replay reads what col.data holds then
    logs, episodes, states, spent = [], [], [], 0.0
    for _ in range(iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col.collect()                                               # eager: the env step takes its counters by value
        col.finish(gamma, lam)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        loop.replay(graph)
        logs.append(loop.log())                                     # the host read of the update phase
        episodes.append(col.episodes())                             # the host read of the collection
        scale, ret = col.obs_state.scale.cpu().numpy(), col.ret_state
        states.append(dict(count=float(col.obs_state.stat[2 * D]), ret_count=float(ret.stat[2]), mean_abs_max=float(abs(scale[:D]).max()),
                           den_max=float(scale[D:].max()), ret_den=float(ret.scale[1])))
    n_pol = len(policy.parameters())
    delta = [float((p.detach() - b).abs().max()) for p, b in zip(policy.parameters() + value.parameters(), before)]
    return dict(logs=logs, episodes=episodes, norm=states, grad_norm=float(upd.adam.state.gnorm), optimiser_steps=int(upd.adam.state.step),
                counter=int(loop.counter), policy_delta=max(delta[:n_pol]), value_delta=max(delta[n_pol:]),
                steps_per_s=B * T * iterations / spent)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    res = run(B, K, N)
    logs, episodes, states = res.pop('logs'), res.pop('episodes'), res.pop('norm')
    for i, (log, ep) in enumerate(zip(logs, episodes)):
        print('iteration %d: observation state count %.4f, largest |mean_f| %.4g, largest den_f %.4g; return state count %.4f, den_f %.4g'
              % (i, states[i]['count'], states[i]['mean_abs_max'], states[i]['den_max'], states[i]['ret_count'], states[i]['ret_den']))
        print('iteration %d: %d episodes ended, return %.3f +- %.3f in [%.3f, %.3f], length %.1f, outcomes %s'
              % (i, ep['episodes'], ep['return_mean'], ep['return_std'], ep['return_min'], ep['return_max'], ep['length_mean'],
                 {k: v for k, v in ep['outcomes'].items() if v and k != 'not_done_yet'}))
        print('  epoch  approx_kl per minibatch' + ' ' * 30 + 'clip_fraction per minibatch')
        for e in range(log['approx_kl'].shape[0]):
            print('  %5d  %s    %s' % (e, ' '.join('%+.3e' % x for x in log['approx_kl'][e]), ' '.join('%.4f' % x for x in log['clip_fraction'][e])))
    last = logs[-1]
    print(dict(res, policy_loss_last=float(last['policy_loss'][-1, -1]), value_loss_last=float(last['value_loss'][-1, -1]),
               entropy_last=float(last['entropy'][-1, -1]), max_ratio_dev_first=float(last['max_ratio_dev'][0, 0])))
