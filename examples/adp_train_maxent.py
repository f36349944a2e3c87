"""adp_train_maxent.py — adp_train_fused.py's training loop under the STOCHASTIC head: maximum-entropy ADP on the model.

    policy = TrainableMLPNet(obs_dim, 2, 64, 'elu', 4)
    opt = torch.optim.Adam(policy.parameters(), lr=1e-3)
    w5 = (-1 / (horizon * B), lam / (horizon * B), 0, 0, 0)              # ADP's loss as weights of out5
    w_logp = alpha / (horizon * B)                                       # J = loss + alpha * mean log pi
    for it in range(iterations):
        loss = rollout_loss_sampled(model, policy, obs0, ref_idx, horizon, w5, w_logp, seed, counter)
        loss.backward()                                                  # the reparameterised gradient, finished in the forward
        opt.step()
        counter += horizon                                               # step t drew with (seed, counter + t): fresh noise next time

eb_policy_rollout_sample runs the sampled rollout and its reverse sweep in three launches whatever the horizon.  The composed path —
per step eb_policy_sample and eb_rollout_step forward, eb_rollout_step_vjp, eb_policy_sample_vjp and eb_mlp_backward back — gives
the same loss and gradient up to the order of the float32 sums; the first iteration prints both.

Run: python examples/adp_train_maxent.py [n_env] [horizon] [iterations]"""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import torch                                                                    # noqa: E402
from env_build_amd.grad import DifferentiableEnvironmentModel                  # noqa: E402
from env_build_amd.policy_grad import TrainableMLPNet, rollout_loss_sampled    # noqa: E402


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


adp = _load('adp_policy_gradient')
mlpnet = _load('adp_train_mlpnet')


def _norm(grads):
    return float(torch.sqrt(sum((g ** 2).sum() for g in grads)))


def run(n_env=1024, horizon=25, iterations=3, task='left', n_veh=None, seed=0, lr=1e-3, hidden=64, lam=10.0, alpha=0.05):
    """-> dict(losses, mean_logp, grad_norm, first): `iterations` Adam steps on one batch of start states through rollout_loss_sampled;
    `first` holds the first iteration's (loss, mean logp, |grad|) of the fused and of the composed path"""
    model = DifferentiableEnvironmentModel(task, mode='training', n_veh=n_veh)
    obs0, ref_idx = adp.start_states(model, n_env, seed)
    policy = TrainableMLPNet(model.obs_dim, 2, hidden, 'elu', 4, name='policy', device=model.device, seed=seed)
    policy.set_obs_scale(mlpnet.obs_scale(model.obs_dim))
    # a sampling policy starts near mean 0 and std exp(-1): the output layer's kernel small, the log-std biases -1 (the head is linear
    # and unbounded; a default initialisation puts exp(log_std) anywhere)
    weights = policy.get_weights()
    weights[-2] = weights[-2] * 0.01
    weights[-1][2:] = -1.0
    policy.set_weights(weights)
    scale = 1.0 / (horizon * n_env)
    w5, w_logp = (-scale, lam * scale, 0.0, 0.0, 0.0), alpha * scale
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    first, losses, mean_logp, grad_norm, counter = {}, [], [], None, 0
    for it in range(iterations):
        for name in (('composed', 'fused') if it == 0 else ('fused',)):
            opt.zero_grad()
            loss, logp = rollout_loss_sampled(model, policy, obs0, ref_idx, horizon, w5, w_logp, seed, counter, fused=None if name == 'fused' else False,
                                              return_logp=True)
            loss.backward()
            grad_norm = _norm([p.grad for p in policy.parameters()])
            if it == 0:
                first[name] = (float(loss.detach()), float(logp.mean()), grad_norm)
        opt.step()
        counter += horizon
        losses.append(float(loss.detach()))
        mean_logp.append(float(logp.mean()))
    return dict(losses=losses, mean_logp=mean_logp, grad_norm=grad_norm, first=first, policy=policy)


def main(argv=None):
    a = [int(v) for v in (sys.argv[1:4] if argv is None else argv)]
    r = run(*a)
    for name in ('fused', 'composed'):
        print('first iteration, %-8s: loss %.6f, mean logp %.6f, |grad| %.6g' % ((name,) + r['first'][name]))
    for it, (v, lp) in enumerate(zip(r['losses'], r['mean_logp'])):
        print('iter %d: loss %.6f, mean logp %.6f' % (it, v, lp))
    print('|grad| of the last step %.4g' % r['grad_norm'])
    return r


if __name__ == '__main__':
    main()
