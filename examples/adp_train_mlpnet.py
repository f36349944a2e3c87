"""adp_train_mlpnet.py — the ADP training step of adp_policy_gradient.py with the project's OWN policy network as the thing trained.

    policy = TrainableMLPNet(obs_dim, 2, 64, 'elu', 4)                 # the MLPNet the shield and the look-ahead evaluate
    policy.set_obs_scale(scale)                                       # the preprocessor, folded into the kernel
    opt = torch.optim.Adam(policy.parameters(), lr=1e-3)              # views of one flat device tensor
    for it in range(iterations):
        loss = rollout_loss(model, lambda o: policy.mode(o, 1.0), obs0, ref_idx)
        loss.backward()                                               # the model step's reverse kernel, then eb_mlp_backward
        opt.step()                                                    # the handle follows on its next launch: no host copy, no sync

There is one copy of the policy: the forward that is differentiated is the one inference runs, bit for bit.  After training the same
handle is switched to fp16 and drives the fused closed-loop rollout (policy_rollout.policy_rollout) — the weights never left the device.

Run: python examples/adp_train_mlpnet.py [n_env] [horizon] [iterations]"""
import importlib.util
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import torch                                                            # noqa: E402
from env_build_amd.dynamics_and_models import EnvironmentModel         # noqa: E402
from env_build_amd.grad import DifferentiableEnvironmentModel          # noqa: E402
from env_build_amd.policy import Policy4Toyota                         # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet                  # noqa: E402
from env_build_amd.policy_rollout import policy_rollout                # noqa: E402

_spec = importlib.util.spec_from_file_location('adp_policy_gradient', os.path.join(HERE, 'adp_policy_gradient.py'))
adp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(adp)


def obs_scale(obs_dim):
    scale = torch.ones(obs_dim)
    scale[3:6] = torch.tensor([0.05, 0.05, 0.01])                       # metres / degrees down to O(1)
    scale[9:] = 0.05
    return scale.numpy()


def as_policy4toyota(net, action_range=1.0):
    """the trained network as the policy head of a Policy4Toyota: what the shield, policy_rollout and HierarchicalDecision take"""
    args = SimpleNamespace(obs_dim=net.input_dim, act_dim=net.output_dim // 2, num_hidden_layers=net.num_hidden_layers,
                           num_hidden_units=net.num_hidden_units, hidden_activation=net.hidden_activation,
                           policy_out_activation=net.output_activation, action_range=action_range, deterministic_policy=True)
    p = Policy4Toyota(args, device=net.device)
    p.policy = net
    p.models = (p.obj_v, net)
    return p


def run(n_env=1024, horizon=25, iterations=3, task='left', n_veh=None, seed=0, lr=1e-3, hidden=64, lookahead=5):
    """-> dict(losses, grad_norm, grads, policy, before, after, rollout): `iterations` Adam steps on one batch of start states with a
    TrainableMLPNet policy, then the fused fp16 look-ahead on the same handle"""
    model = DifferentiableEnvironmentModel(task, mode='training', n_veh=n_veh)
    obs0, ref_idx = adp.start_states(model, n_env, seed)
    policy = TrainableMLPNet(model.obs_dim, 2, hidden, 'elu', 4, name='policy', device=model.device, seed=seed)
    policy.set_obs_scale(obs_scale(model.obs_dim))
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    before = policy.get_weights()
    losses, grad_norm, grads = [], None, None
    for _ in range(iterations):
        opt.zero_grad()
        loss = adp.rollout_loss(model, lambda o: policy.mode(o, 1.0), obs0, ref_idx, horizon)
        loss.backward()
        grads = [p.grad.detach().clone() for p in policy.parameters()]
        grad_norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads)))
        opt.step()
        losses.append(float(loss.detach()))
    # the trained weights in the loop: same handle, fp16, `lookahead` steps of policy -> model in one launch
    policy.set_precision('fp16')
    plain = EnvironmentModel(task, mode='training', n_veh=model.veh_num)
    plain.reset(obs0, ref_idx)
    rollout = policy_rollout(plain, as_policy4toyota(policy), obs0, lookahead, want=('out5', 'actions'))
    return dict(losses=losses, grad_norm=grad_norm, grads=grads, policy=policy, before=before, after=policy.get_weights(), rollout=rollout,
                obs0=obs0, ref_idx=ref_idx, task=task, n_veh=model.veh_num, lookahead=lookahead)


if __name__ == '__main__':
    a = [int(v) for v in sys.argv[1:4]]
    r = run(*a)
    print('ADP step(s) on the GPU with a TrainableMLPNet: loss %s, |grad| of the last step %.4g; fp16 look-ahead fused: %s, safe %d of %d'
          % (' -> '.join('%.4f' % v for v in r['losses']), r['grad_norm'], r['rollout']['fused'],
             int(r['rollout']['safe'].t.sum()), len(r['obs0'])))
