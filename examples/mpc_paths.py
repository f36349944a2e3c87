"""mpc_paths.py — receding-horizon MPC that optimises a tape on EVERY path of the task and compares them, each control step.

The reference's decision loop scores its candidate paths by the value of acting well on each (hier_decision.py:113-121).  The
model-cost twin is OpenLoopMPC.solve_paths: one start per path, candidate p on path p from the row's tracking error on that path, all
optimised together — the P gradients of an iteration are ONE eb_rollout_tape_cand_vjp launch from the shared scene
(include/envbuild_cand_grad.h) — and the best path per env returned.  The loop is that of examples/mpc_open_loop.py:

    mpc = OpenLoopMPC(env.env_model, horizon=25)
    u, J, info = mpc.solve_paths(obs)                      # info['path_index'] [B], info['J_paths'] [P, B], info['u_paths'] [P, H, B, 2]
    obs, reward, done, _ = env.step(u[0])                  # apply the first action of the best path's tape
    u_init = torch.stack([mpc.warm_start(v) for v in info['u_paths']])

Switching the env's own path to info['path_index'] (with the hysteresis of hier_decision.py:121) is the caller's decision; this
example reports how often the best path differs from the one the env follows.

Run: python examples/mpc_paths.py [n_env] [control_steps] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                               # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end        # noqa: E402
from env_build_amd.mpc import OpenLoopMPC                  # noqa: E402


def run(n_env=256, control_steps=5, iterations=20, horizon=25, task='left', seed=0):
    """-> dict(J_first [B], J0_first [B]: the best path's zero-tape cost at the first solve, J_last [B], path_first [B], path_last [B],
    other_path: env-steps whose best path is not the env's own, reward_sum [B], launches)"""
    if n_env < 2:
        raise ValueError('a batch of envs: n_env >= 2')
    env = CrossroadEnd2end(task, n_env=n_env)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    mpc = OpenLoopMPC(env.env_model, horizon=horizon, iterations=iterations)
    ref = env._ref_index_out().t                           # the path every env follows
    u_init, first, info, J = None, None, None, None
    reward_sum = torch.zeros(n_env, device=env.device)
    other = 0
    for _ in range(control_steps):
        u, J, info = mpc.solve_paths(obs.t, u_init=u_init)
        if first is None:
            J0 = info['J_history'][0].gather(0, info['path_index'].view(1, -1))[0]
            first = dict(J_first=J.clone(), J0_first=J0, path_first=info['path_index'].clone())
        other += int((info['path_index'] != ref.long()).sum())
        obs, reward, done, step_info = env.step(u[0].contiguous())
        reward_sum += reward.t
        ref = step_info['ref_index'].t
        u_init = torch.stack([mpc.warm_start(v) for v in info['u_paths']])
    return dict(J_last=J, path_last=info['path_index'], other_path=other, reward_sum=reward_sum, launches=mpc.launches, **first)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:4]]
    r = run(*a)
    print('per-path MPC on the GPU: first solve J %.2f -> %.2f (mean over envs, best path), last solve %.2f; best path != own path on '
          '%d env-steps; %d launches' % (float(r['J0_first'].mean()), float(r['J_first'].mean()), float(r['J_last'].mean()),
                                         r['other_path'], r['launches']))
