"""mpc_open_loop.py — receding-horizon MPC for a batch of envs: the loop of the reference's mpc/main.py:551-576, batched.

The reference solves one ego's 25 x 2 open-loop actions with SLSQP and finite differences, applies the first action, and solves
again.  Here every env of a CrossroadEnd2end batch is solved at once by env_build_amd.mpc.OpenLoopMPC — projected gradient on the
model's own cost, one eb_rollout_tape_vjp launch per evaluation — and the next solve starts from the shifted tape (the warm start
mpc/main.py:571 left commented out):

    env = CrossroadEnd2end('left', n_env=256)
    obs = env.reset()
    mpc = OpenLoopMPC(env.env_model, horizon=25)
    u, J, info = mpc.solve(obs, ref_indexes=ref)          # u [25, B, 2] in [-1, 1]
    obs, reward, done, info = env.step(u[0])              # apply the first action
    u_init = mpc.warm_start(u)

Run: python examples/mpc_open_loop.py [n_env] [control_steps] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                               # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end        # noqa: E402
from env_build_amd.mpc import OpenLoopMPC                  # noqa: E402


def run(n_env=256, control_steps=5, iterations=20, horizon=25, task='left', seed=0):
    """-> dict(J_first [B]: cost of the first solve, J0_first [B]: of the zero tape there, J_last [B], reward_sum [B], launches)"""
    if n_env < 2:
        raise ValueError('a batch of envs: n_env >= 2')
    env = CrossroadEnd2end(task, n_env=n_env)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    mpc = OpenLoopMPC(env.env_model, horizon=horizon, iterations=iterations)
    ref = env._ref_index_out().t                           # the path every env follows (info['ref_index'] after a step)
    u_init, J_first, J0_first, J = None, None, None, None
    reward_sum = torch.zeros(n_env, device=env.device)
    for _ in range(control_steps):
        u, J, info = mpc.solve(obs.t, ref_indexes=ref, u_init=u_init)
        if J_first is None:
            J_first, J0_first = J.clone(), info['J_history'][0].clone()
        obs, reward, done, step_info = env.step(u[0].contiguous())
        reward_sum += reward.t
        ref = step_info['ref_index'].t
        u_init = mpc.warm_start(u)
    return dict(J_first=J_first, J0_first=J0_first, J_last=J, reward_sum=reward_sum, launches=mpc.launches)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:4]]
    r = run(*a)
    print('open-loop MPC on the GPU: first solve J %.2f -> %.2f (mean over envs), last solve %.2f; %d launches'
          % (float(r['J0_first'].mean()), float(r['J_first'].mean()), float(r['J_last'].mean()), r['launches']))
