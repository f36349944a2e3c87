"""policy_lookahead.py — multi_ego's 20-step look-ahead (multi_ego.py:187-209) for a batch of start states in ONE launch.

The reference rolls the model forward under the policy for 20 steps, adds real_punish_term up and calls the start state unsafe when
the sum turns positive — and keeps nothing else.  env_build_amd.policy_rollout returns the per-step outputs of the same loop; with an
fp16 policy the policy network and the model step run fused in one kernel (include/envbuild_policy_rollout.h), the rows staying on
the compute unit for the whole horizon:

    model = EnvironmentModel('left', 0, mode='selecting')
    policy = LoadPolicy(exp_dir, iteration)                  # config.json with "policy_precision": "fp16"
    out = policy_rollout(model, policy, obses, steps=20, path_index=1, penalty='real_punish_term', want=('out5',))
    out['out5_steps']                                        # [20, 5, B]: rewards, punish_term_for_training, real_punish_term, ...
    out['safe'], out['punish'], out['fused']                 # the shield's flag and sum; whether the one-launch kernel ran

Run: python examples/policy_lookahead.py [--batch B] [--n-veh N] [--steps H] [--task left|straight|right]"""
import argparse
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                              # noqa: E402
from env_build_amd.dynamics_and_models import EnvironmentModel, _unwrap   # noqa: E402
from env_build_amd.policy import LoadPolicy                               # noqa: E402
from env_build_amd.policy_rollout import policy_rollout                   # noqa: E402
from env_build_amd.synthetic import assemble_obs, make_rollout_inputs     # noqa: E402


def run(batch=256, n_veh=8, steps=20, task='left', path_index=1, seed=0):
    """-> policy_rollout's dict for `batch` synthetic start states under a randomly initialised fp16 policy"""
    model = EnvironmentModel(task, 0, mode='selecting', n_veh=n_veh)
    D = model.obs_dim
    scale = [0.2] * 6 + [1., 1 / 30., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * n_veh
    policy = LoadPolicy(args=SimpleNamespace(obs_dim=D, act_dim=2, num_hidden_layers=2, num_hidden_units=256, hidden_activation='elu',
                                             policy_out_activation='linear', action_range=1.0, deterministic_policy=True,
                                             obs_preprocess_type='scale', obs_scale=scale, policy_precision='fp16'))
    inp = make_rollout_inputs(task, batch, n_veh, 1, seed=seed)
    ego = inp['ego']
    model.ref_path.set_path(path_index)
    trk = _unwrap(model.ref_path.tracking_error_vector(ego[:, 3], ego[:, 4], ego[:, 5], ego[:, 0], 0))
    obses = assemble_obs(ego, trk.detach().cpu().numpy().reshape(batch, 3), inp['veh'])
    out = policy_rollout(model, policy, obses, steps, path_index=path_index, penalty='real_punish_term', want=('out5',))
    torch.cuda.synchronize()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--n-veh', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--task', default='left', choices=('left', 'straight', 'right'))
    a = ap.parse_args(argv)
    out = run(a.batch, a.n_veh, a.steps, a.task)
    out5 = _unwrap(out['out5_steps']).cpu()
    print('%d-step look-ahead for %d start states (%s, %d vehicle slots); fused: %s' % (a.steps, a.batch, a.task, a.n_veh, out['fused']))
    for t in range(a.steps):
        real = out5[t, 2]
        print('step %2d: real_punish_term mean %.4f max %.4f, rows penalised %d' % (t, float(real.mean()), float(real.max()), int((real > 0).sum())))
    safe = _unwrap(out['safe'])
    print('safe: %d of %d (accumulated penalty max %.4f)' % (int(safe.sum()), a.batch, float(_unwrap(out['punish']).max())))


if __name__ == '__main__':
    main()
