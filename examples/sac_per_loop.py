"""sac_per_loop.py — examples/sac_env_loop.py with prioritised experience replay (env_build_amd.per, include/envbuild_per.h): the ring
carries a radix-32 sum tree on the device, the collector gives every pushed slot the largest priority seen, and the captured SAC update
draws in proportion to the priorities, weighs the critics' cotangents and writes the new TD errors back — all inside the one graph.

    buf = PrioritizedReplayBuffer(capacity, D, A, device)
    col = Collector(env, policy, buf, action_range, seed=seed)         # offpolicy.Collector's three launches + the range route's
    sac = SAC(policy, q1, q2, buf, batch, alpha=0.6, beta0=0.4, beta_step=..., eps=1e-6, ...)
    col.random_steps(warmup)
    graph = sac.capture()                                              # sac.KERNELS kernel nodes
    for every iteration:
        col.step(); sac.replay(graph); sac.log()

beta anneals from beta0 to 1 over the iterations on the device: the graph reads the draw counter.  Nothing here claims that it learns well.
Run: python examples/sac_per_loop.py [--n-env 4096] [--iterations 8] [--warmup 4] [--batch 4096] [--capacity 1048576] [--hidden 256]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np                                                  # noqa: E402
from env_build_amd import _capi                                     # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end                 # noqa: E402
from env_build_amd.per import SAC, Collector, PrioritizedReplayBuffer   # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet               # noqa: E402


def main(argv=None):
    """-> SAC.log() per iteration"""
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=4096)
    ap.add_argument('--iterations', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--capacity', type=int, default=1 << 20)
    ap.add_argument('--hidden', type=int, default=256)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    env = CrossroadEnd2end('left', n_env=args.n_env, auto_reset=True, copy_outputs=False, max_episode_steps=200)
    env.seed(args.seed)
    env.reset()
    env.reset()
    dev, D, A = env.device, env.obs_dim, env.action_number
    policy = TrainableMLPNet(D, 2, args.hidden, 'elu', 2 * A, output_activation='linear', name='policy', device=dev, seed=args.seed)
    q1 = TrainableMLPNet(D + A, 2, args.hidden, 'elu', 1, output_activation='linear', name='q1', device=dev, seed=args.seed + 1)
    q2 = TrainableMLPNet(D + A, 2, args.hidden, 'elu', 1, output_activation='linear', name='q2', device=dev, seed=args.seed + 2)
    scale = [0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num
    policy.set_obs_scale(scale)
    q1.set_obs_scale(scale + [1.] * A)
    q2.set_obs_scale(scale + [1.] * A)
    buf = PrioritizedReplayBuffer(max(args.capacity, args.n_env), D, A, dev)
    col = Collector(env, policy, buf, 1.0, seed=args.seed)
    sac = SAC(policy, q1, q2, buf, args.batch, alpha=0.6, beta0=0.4, beta_step=0.6 / max(args.iterations - 1, 1), eps=1e-6, gamma=0.99,
              tau=0.005, lr=3e-4, action_range=1.0, seed=args.seed)
    col.random_steps(args.warmup)
    graph = sac.capture()                                           # nothing runs; every replay reads what the ring and the tree hold then
    logs = []
    for i in range(args.iterations):
        col.step()
        sac.replay(graph)
        log = sac.log()
        codes = env.done_code.cpu().numpy()
        ended = {_capi.DONE_NAMES[int(c)]: int(n) for c, n in zip(*np.unique(codes[codes != 0], return_counts=True))}
        print('iteration %d: %d transitions in the ring; weighted critic losses %.4f %.4f, actor loss %.4f, alpha %.4f, mean weight %.3f '
              'at beta %.3f; episodes ended at this step: %s' % (i, len(buf), log['critic1_loss'], log['critic2_loss'], log['actor_loss'],
                                                                 log['alpha'], log['weight'], log['beta'], ended or 'none'))
        logs.append(log)
    return logs


if __name__ == '__main__':
    main()
