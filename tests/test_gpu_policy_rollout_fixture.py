"""GPU (-m gpu): the closed-loop gradient kernels against a yardstick from outside the project.  eb_policy_rollout_grad and
eb_policy_rollout_sample are launched on the inputs of the G21 fixtures (tests/golden/g21_policy_rollout_grad_<task>.npz: the
reference's model in closed loop with a torch MLP, differentiated by torch.autograd in float64 and float32) and held to them:

  forward    out5_steps, actions_steps, logp_steps against the reference's float32 run, rtol 1e-5 / atol 5e-6;
  gradients  g_obs0 and g_actions_steps per column, g_params per tensor, against the float64 run:
             |got - ref64| <= 4 E + 2^-20 max |ref64|, E the reference's own float32 error (tests/_grad_cases.py's bar, the one
             G15 / G16 / G18 hold the env VJP to);
  façade     once per task, rollout_loss(...).backward() and rollout_loss_sampled(...).backward() on a TrainableMLPNet: the
             parameters' .grad meets the same bar.

What the "equals the loop" tests cannot see — which columns re-enter lambda, whether the tracking columns carry gradient back into the
ego state, where stop_gradient cuts, the w_logp path through the sampling head, the obs scale inside the loop — is wrong here by
1e-2 of a tensor's maximum or more, four orders above the bar.  Reads tests/golden only.  Measured error / tolerance: DESIGN §5 (G21)."""
import numpy as np
import pytest

from tests import _policy_rollout_fixture as F
from tests import _policy_rollout_grad as H
from tests import _policy_rollout_sample as S
from tests._helpers import close
from tests._policy import same, split_params

pytestmark = pytest.mark.gpu


def launch(c, dev, m):
    if c.sampled:
        return S.entry(dev, m, c.obs0, c.steps, c.w5, c.w_logp, c.ref_idx(), c.path_id(), c.ar, eps=c.eps)
    return H.entry(dev, m, c.obs0, c.steps, c.w5, c.ref_idx(), c.path_id(), c.ar)


def show_worst(what):
    for key in sorted(k for k in F.WORST if k.startswith(what)):
        print('%-46s worst error / tolerance %.3f' % (key, F.WORST[key]))


@pytest.mark.parametrize('c', F.all_cases(), ids=F.case_id)
def test_entry_meets_the_reference_closed_loop(c):
    dev = H.model(c.task, c.n_veh, c.mode)
    m = dev.make_mlp(*c.net_args())
    assert (S.supported if c.sampled else H.supported)(dev, m)[0] == 1
    assert H.param_count(dev, m) == sum(w.size for w in c.weights)
    got = launch(c, dev, m)
    what = 'G21 %s %s' % (c.task, c.name)
    close(got['out5'], c['out5_steps'], F.RTOL, F.ATOL, what + ' out5')
    close(got['actions'], c['actions_steps'], F.RTOL, F.ATOL, what + ' actions')
    if c.sampled:
        close(got['logp'], c['logp_steps'], F.RTOL, F.ATOL, what + ' logp')
        assert same(got['eps'], c.eps)
    assert np.array_equal(got['obs'][-1], got['last']) and np.isfinite(got['last']).all()
    F.check_rows(c, got['g_obs0'], got['g_actions'], what)
    F.check_params(c, split_params(got['g_params'], c.dims), what)
    show_worst(what)
    dev.api.mlp_destroy(m)


@pytest.mark.parametrize('task', F.TASKS)
def test_facade_backward_meets_the_reference_closed_loop(task):
    import torch
    from env_build_amd import policy_grad
    from env_build_amd.grad import DifferentiableEnvironmentModel
    by_name = {c.name: c for c in F.cases(task)}
    det, sto = by_name['det_H5'], by_name['sto_H5']
    model = DifferentiableEnvironmentModel(task, 0, mode='training', n_veh=det.n_veh)
    pol = policy_grad.TrainableMLPNet(det.D, det.dims[1], det.dims[2], det.hact, 4, name='policy', output_activation='linear')
    pol.set_weights(det.weights)
    pol.set_obs_scale(det.scale)
    ob = torch.from_numpy(det.obs0).to(model.device)
    ri = torch.from_numpy(det.ref_idx().astype(np.int32)).to(model.device)

    def weighted(c):
        """J's cost part from the fixture's float32 forward, in float64, and the sum of its terms' magnitudes"""
        terms = c['out5_steps'].astype(np.float64) * np.asarray(c.w5, np.float64).reshape(1, 5, 1)
        return terms.sum(), np.abs(terms).sum(), terms.size

    def grads():
        out = [p.grad.detach().cpu().numpy() for p in pol.parameters()]
        for p in pol.parameters():
            p.grad = None
        return out
    # every out5 is within rtol 1e-5 / atol 5e-6 of the fixture's; the float32 sums of cost add (terms - 1) 2^-24 of the magnitudes
    bound = lambda c, mag, terms: 1e-5 * mag + 5e-6 * np.abs(c.w5).sum() * c.steps * c.n + terms * 2.0 ** -24 * mag
    what = 'G21 %s det_H5 rollout_loss' % task
    loss = policy_grad.rollout_loss(model, pol, ob, ri, det.steps, det.w5, action_range=det.ar)
    loss.backward()
    J, mag, terms = weighted(det)
    assert abs(float(loss) - J) <= bound(det, mag, terms) and float(loss) != 0.0
    F.check_params(det, grads(), what)
    show_worst(what)

    assert sto.weights is not det.weights and all(np.array_equal(a, b) for a, b in zip(sto.weights, det.weights))     # the same net
    what = 'G21 %s sto_H5 rollout_loss_sampled' % task
    loss, logp = policy_grad.rollout_loss_sampled(model, pol, ob, ri, sto.steps, sto.w5, sto.w_logp, seed=0, counter=0, eps=sto.eps,
                                                  action_range=sto.ar, return_logp=True)
    loss.backward()
    close(logp.cpu().numpy(), sto['logp_steps'], F.RTOL, F.ATOL, what + ' logp')
    J, mag, terms = weighted(sto)
    lp = sto.w_logp * sto['logp_steps'].astype(np.float64)
    slack = abs(sto.w_logp) * (1e-5 * np.abs(sto['logp_steps']).sum() + 5e-6 * lp.size) + lp.size * 2.0 ** -24 * np.abs(lp).sum()
    assert abs(float(loss) - (J + lp.sum())) <= bound(sto, mag, terms) + slack
    F.check_params(sto, grads(), what)
    show_worst(what)
