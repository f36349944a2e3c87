"""adp_policy_gradient.py — one ADP training step against the differentiable model: the loop a model-based RL trainer writes.

The reference trains its policy by back-propagating the rollout's `rewards` and `punish_term_for_training` through
EnvironmentModel.rollout_out (DAM:118-126).  With env_build_amd the same loop runs on an MI355X: the forward of every step is the
fused rollout kernel, its backward the hand-written reverse kernel (csrc/eb_rollout_vjp.hip), and the policy is any torch module.

    model = DifferentiableEnvironmentModel(task, mode='training', n_veh=n_veh)
    model.reset(obs0, ref_idx)
    for t in range(25):
        obs, rewards, punish, *_ = model.rollout_out(policy(obs))     # one launch
        loss += (-rewards + lam * punish).mean()
    loss.backward()                                                   # one reverse launch per step, then the policy's own backward
    optimiser.step()

Run: python examples/adp_policy_gradient.py [n_env] [horizon] [iterations]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch                                                            # noqa: E402
from env_build_amd.grad import DifferentiableEnvironmentModel          # noqa: E402
from env_build_amd.synthetic import make_rollout_inputs                # noqa: E402


def start_states(model, n_env, seed=0):
    """Synthetic start states [B, D] (env_build_amd.synthetic) with their tracking columns, and the path index per env."""
    dev = model.device
    inp = make_rollout_inputs(model.task, n_env, model.veh_num, 1, seed=seed, n_future=model.num_future_data)
    ego, ref = torch.from_numpy(inp['ego']).to(dev), torch.from_numpy(inp['ref_idx']).to(dev)
    trk = model.ref_path.tracking_error_vector_batched(ego[:, 3].contiguous(), ego[:, 4].contiguous(), ego[:, 5].contiguous(),
                                                       ego[:, 0].contiguous(), model.num_future_data, ref_indexes=ref).t
    return torch.cat([ego, trk, torch.from_numpy(inp['veh']).to(dev)], 1).contiguous(), ref


def make_policy(obs_dim, device, hidden=64, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(obs_dim, hidden), torch.nn.ELU(), torch.nn.Linear(hidden, hidden), torch.nn.ELU(),
                               torch.nn.Linear(hidden, 2), torch.nn.Tanh()).to(device)


def rollout_loss(model, policy, obs0, ref_idx, horizon=25, lam=10.0, obs_scale=None):
    """mean over envs and steps of -rewards + lam * punish_term_for_training, on the autograd graph"""
    model.reset(obs0, ref_idx)
    obs, loss = obs0, 0.0
    for _ in range(horizon):
        x = obs if obs_scale is None else obs * obs_scale
        obs, rewards, punish = model.rollout_out(policy(x))[:3]
        loss = loss + (-rewards + lam * punish).mean()
    return loss / horizon


def run(n_env=1024, horizon=25, iterations=1, task='left', n_veh=None, seed=0, lr=1e-3):
    """-> dict(losses, grad_norm): `iterations` optimiser steps on one batch of start states"""
    model = DifferentiableEnvironmentModel(task, mode='training', n_veh=n_veh)
    obs0, ref_idx = start_states(model, n_env, seed)
    policy = make_policy(model.obs_dim, model.device, seed=seed)
    scale = torch.ones(model.obs_dim, device=model.device)
    scale[3:6] = torch.tensor([0.05, 0.05, 0.01], device=model.device)     # metres / degrees down to O(1)
    scale[9:] = 0.05
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    losses, grad_norm = [], None
    for _ in range(iterations):
        opt.zero_grad()
        loss = rollout_loss(model, policy, obs0, ref_idx, horizon, obs_scale=scale)
        loss.backward()
        grad_norm = float(torch.sqrt(sum((p.grad ** 2).sum() for p in policy.parameters())))
        opt.step()
        losses.append(float(loss.detach()))
    return dict(losses=losses, grad_norm=grad_norm)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:4]]
    r = run(*a)
    print('ADP step(s) on the GPU: loss %s, |grad| of the last step %.4g'
          % (' -> '.join('%.4f' % v for v in r['losses']), r['grad_norm']))
