"""mpc_candidates.py — receding-horizon MPC for a batch of envs with candidate-tape launches: examples/mpc_open_loop.py with the
line search fused and two starts per solve.

The loop is the reference's mpc/main.py:551-576, batched.  Two things ask "what do these K tapes cost from this one state?" and are
answered by ONE eb_rollout_tape_cand launch each (include/envbuild_cand.h: the scene's vehicles advance once for all K tapes):

  * the Armijo trials of an iteration (fused_line_search=True): 2 launches per iteration instead of 4, the same bits;
  * the starts of a solve: the shifted tape of the last solve (the warm start mpc/main.py:571 left commented out) and the zero tape
    (mpc/main.py:550) — every env starts from whichever costs less.

    mpc = OpenLoopMPC(env.env_model, horizon=25, fused_line_search=True)
    u, J, info = mpc.solve(obs, ref_indexes=ref, u_init=torch.stack([mpc.warm_start(u), torch.zeros_like(u)]))
    info['start_index']                                   # [B]: 0 = warm start, 1 = zero tape

Run: python examples/mpc_candidates.py [n_env] [control_steps] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                               # noqa: E402
from env_build_amd.endtoend import CrossroadEnd2end        # noqa: E402
from env_build_amd.mpc import OpenLoopMPC                  # noqa: E402


def run(n_env=256, control_steps=5, iterations=20, horizon=25, task='left', seed=0):
    """-> dict(J_first [B]: cost of the first solve, J0_first [B]: of its start, J_last [B], J0_last [B], reward_sum [B],
    zero_starts: how many (env, solve) pairs started from the zero tape although a warm start was offered, launches)"""
    if n_env < 2:
        raise ValueError('a batch of envs: n_env >= 2')
    env = CrossroadEnd2end(task, n_env=n_env)
    env.seed(seed)
    env.reset()
    obs = env.reset()
    mpc = OpenLoopMPC(env.env_model, horizon=horizon, iterations=iterations, fused_line_search=True)
    ref = env._ref_index_out().t                           # the path every env follows (info['ref_index'] after a step)
    zero = torch.zeros((horizon, n_env, 2), dtype=torch.float32, device=env.device)
    u_init, J_first, J0_first, J, J0, zero_starts = None, None, None, None, None, 0
    reward_sum = torch.zeros(n_env, device=env.device)
    for _ in range(control_steps):
        u, J, info = mpc.solve(obs.t, ref_indexes=ref, u_init=u_init)
        J0 = info['J_history'][0].clone()
        if J_first is None:
            J_first, J0_first = J.clone(), J0
        else:
            zero_starts += int((info['start_index'] == 1).sum())
        obs, reward, done, step_info = env.step(u[0].contiguous())
        reward_sum += reward.t
        ref = step_info['ref_index'].t
        u_init = torch.stack([mpc.warm_start(u), zero])    # two starts: one candidate launch scores both
    return dict(J_first=J_first, J0_first=J0_first, J_last=J, J0_last=J0, reward_sum=reward_sum, zero_starts=zero_starts,
                launches=mpc.launches)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:4]]
    r = run(*a)
    print('open-loop MPC with candidate launches: first solve J %.2f -> %.2f (mean over envs), last solve %.2f; %d launches; '
          '%d solves started from the zero tape' % (float(r['J0_first'].mean()), float(r['J_first'].mean()),
                                                    float(r['J_last'].mean()), r['launches'], r['zero_starts']))
