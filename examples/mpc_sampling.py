"""mpc_sampling.py — receding-horizon SAMPLING MPC (MPPI) for a batch of envs: the loop of examples/mpc_open_loop.py with
env_build_amd.mpc.SamplingMPC, alone and as the global stage in front of the gradient solver.

The model's cost is non-convex (collision discs), so a descent ends in the basin it starts in.  SamplingMPC draws n_samples perturbed
tapes per env and iteration around a nominal tape, scores them from the shared scene and moves the nominal to their soft-min
average — one eb_rollout_tape_sample launch per iteration, no gradient, no noise tensor in memory:

    env = CrossroadEnd2end('left', n_env=256)
    obs = env.reset()
    smpc = SamplingMPC(env.env_model, horizon=25, n_samples=256, iterations=6)
    u, J, info = smpc.solve(obs, ref_indexes=ref, counter=k)      # u [25, B, 2] in [-1, 1]
    obs, reward, done, info = env.step(u[0])                      # apply the first action
    u_init, k = smpc.warm_start(u), info['counter_next']

    hybrid = SamplingMPC(env.env_model, horizon=25, polish=OpenLoopMPC(env.env_model, horizon=25, iterations=20))

Run: python examples/mpc_sampling.py [n_env] [control_steps] [iterations] [polish: 0 / 1]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                               # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end        # noqa: E402
from env_build_amd.mpc import OpenLoopMPC, SamplingMPC     # noqa: E402


def run(n_env=256, control_steps=5, iterations=6, polish=False, n_samples=256, polish_iterations=10, horizon=25, task='left', seed=0):
    """-> dict(J_first [B]: cost of the first solve, J0_first [B]: of the zero tape there, J_last [B], reward_sum [B], launches)"""
    if n_env < 2:
        raise ValueError('a batch of envs: n_env >= 2')
    env = CrossroadEnd2end(task, n_env=n_env)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    descent = OpenLoopMPC(env.env_model, horizon=horizon, iterations=polish_iterations) if polish else None
    smpc = SamplingMPC(env.env_model, horizon=horizon, n_samples=n_samples, iterations=iterations, seed=seed, polish=descent)
    ref = env._ref_index_out().t                           # the path every env follows (info['ref_index'] after a step)
    u_init, J_first, J0_first, J = None, None, None, None
    counter, launches = 0, 0
    reward_sum = torch.zeros(n_env, device=env.device)
    for _ in range(control_steps):
        u, J, info = smpc.solve(obs.t, ref_indexes=ref, u_init=u_init, counter=counter)
        counter = info['counter_next']                     # fresh noise at every control step
        launches += info['launches']
        if J_first is None:
            J_first, J0_first = J.clone(), info['J_history'][0].clone()
        obs, reward, done, step_info = env.step(u[0].contiguous())
        reward_sum += reward.t
        ref = step_info['ref_index'].t
        u_init = smpc.warm_start(u)
    return dict(J_first=J_first, J0_first=J0_first, J_last=J, reward_sum=reward_sum, launches=launches)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:5]]
    if len(a) == 4:
        a[3] = bool(a[3])
    r = run(*a)
    print('sampling MPC on the GPU: first solve J %.2f -> %.2f (mean over envs), last solve %.2f; %d launches'
          % (float(r['J0_first'].mean()), float(r['J_first'].mean()), float(r['J_last'].mean()), r['launches']))
