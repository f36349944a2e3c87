"""sample_env_loop.py — the batched `CrossroadEnd2end` loop of vector_env_loop.py driven by SAMPLED actions: what the reference's
off-policy sampler does with `Policy4Toyota(deterministic_policy=False)` (utils/policy.py:85-96), one env at a time, as two launches
per step for thousands of envs.

    policy = LoadPolicy(args=dict(..., deterministic_policy=False))    # same class, the stochastic branch
    policy.policy.seed(0)                                             # the draws repeat: call k draws from (seed, k)
    actions, logp = policy.policy.compute_action(obs)                 # ONE launch (csrc/eb_policy_sample.hip): the network, the
                                                                      # tanh-Gaussian sample and its log-probability; the noise is
                                                                      # a function of (seed, call, row) and never exists in memory
    obs, reward, done, info = env.step(actions)                       # ONE launch (csrc/eb_env_step.hip), finished envs reset in it

Everything below the Python calls runs in libenvbuild_hip.so; there is no CPU path.
Run: python examples/sample_env_loop.py [n_env] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                               # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end        # noqa: E402
from env_build_amd.policy import LoadPolicy                # noqa: E402


def run(n_env=4096, steps=200, task='left', seed=0, num_hidden_units=256, warmup=10):
    """-> dict(episodes, mean_return, mean_logp, steps_per_s) of a randomly initialised stochastic policy"""
    env = CrossroadEnd2end(task, n_env=n_env, auto_reset=True, copy_outputs=False)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    policy = LoadPolicy(args=dict(obs_dim=env.obs_dim, act_dim=2, num_hidden_layers=2, num_hidden_units=num_hidden_units,
                                  hidden_activation='elu', policy_out_activation='linear', action_range=1.0,
                                  deterministic_policy=False, obs_preprocess_type='scale',
                                  obs_scale=[0.2, 1., 2., 1 / 30., 1 / 30., 1 / 180.] + [1., 1 / 15., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * env.veh_num),
                        device=env.device)
    policy.policy.seed(seed)
    ret = torch.zeros(n_env, device=env.device)
    finished_ret, episodes, logp_sum = (torch.zeros((), device=env.device) for _ in range(3))
    t0 = None
    for k in range(-warmup, steps):
        if k == 0:
            ret.zero_(); finished_ret.zero_(); episodes.zero_(); logp_sum.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        actions, logp = policy.policy.compute_action(obs)  # DevArrays [B, 2] and [B]
        obs, reward, done, info = env.step(actions)
        logp_sum += logp.t.sum()
        ret += reward.t
        fin = env.done_code != 0
        finished_ret += (ret * fin).sum()
        episodes += fin.sum()
        ret = torch.where(fin, torch.zeros_like(ret), ret)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = float(episodes)
    return dict(episodes=int(n), mean_return=float(finished_ret) / max(n, 1.0), mean_logp=float(logp_sum) / (n_env * steps),
                steps_per_s=n_env * steps / dt)


if __name__ == '__main__':
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    print(run(B, K))
