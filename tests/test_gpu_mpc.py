"""GPU (-m gpu): OpenLoopMPC (env_build_amd/mpc.py) — batched projected-gradient MPC on the model's own cost, one
eb_rollout_tape_vjp launch per evaluation — on the start states of the g17 fixtures (scripts/gen_golden_mpc.py: the reference's
rollout_out in float64, SciPy SLSQP as mpc/main.py:554-560).

Exact, on every row: u in [-1, 1]; the returned J is, bit for bit, mpc.cost_from_out5 of an independent eb_rollout_tape over the
returned u; J never increases over the iterations; J <= J(0); a second solve repeats its bits.
Against the reference's optimiser: a row AGREES when J_hip <= J_ref + 0.1 — 0.1 is the reference's own stopping tolerance
(tol=1e-1, mpc/main.py:558), not a tuned figure; the cost is non-convex (collision discs), so at most ONE QUARTER of a file's rows
may disagree (the fixtures hold rows on which the reference alone disagrees with itself on at most that share).

Measured on an MI355X (60 iterations, the defaults), rows that disagree: left 2 of 9, straight 2 of 16, right 3 of 16; the float64
run of the same lines on the reference's cost: 2 of 9, 1 of 16, 3 of 16."""
import numpy as np
import pytest

from tests._grad_cases import TASKS
from tests._tape import load_example, mpc_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('task', TASKS)
def test_solver_invariants_and_agreement_with_the_reference_optimiser(task):
    import torch
    from env_build_amd.mpc import cost_from_out5
    z, model, mpc, obs0, ref = mpc_setup(task)
    B = obs0.shape[0]
    u, J, info = mpc.solve(obs0, ref_indexes=ref)
    assert u.shape == (25, B, 2) and J.shape == (B,) and torch.isfinite(J).all()
    assert float(u.abs().max()) <= 1.0
    # J is the cost of the returned tape: an independent eb_rollout_tape, the same summation
    model.reset(obs0, ref)
    _final, out5 = model.rollout_tape(u)
    out5 = out5.t if hasattr(out5, 't') else out5
    J_check = cost_from_out5(out5, mpc.weights)
    assert torch.equal(J.view(torch.int32), J_check.view(torch.int32))
    hist = info['J_history']
    assert hist.shape[0] == info['iterations'] + 1 and bool((hist[1:] <= hist[:-1]).all())       # accepted steps only
    assert torch.equal(hist[-1], J)
    # J(0): the zero tape, in float32 on the device and in float64 in the fixture (a sanity check that both sides evaluate the same
    # cost, not a precision claim: rtol 1e-4 next to atol 1e-3 is an order above the rtol 1e-5 + atol 5e-6 every out5 term is held to,
    # for a weighted sum of 50 of them with weights up to 10)
    J0 = hist[0].double().cpu().numpy()
    assert np.allclose(J0, z['J0'], rtol=1e-4, atol=1e-3)
    assert bool((J <= hist[0]).all())
    assert info['launches'] == 1 + info['iterations'] * info['launches_per_iteration']
    # a second solve from the same inputs repeats its bits
    u2, J2, _ = mpc.solve(obs0, ref_indexes=ref)
    assert torch.equal(u2.view(torch.int32), u.view(torch.int32)) and torch.equal(J2.view(torch.int32), J.view(torch.int32))
    # against SLSQP
    Jh = J.double().cpu().numpy()
    agree = Jh <= z['J_ref'] + 0.1
    for r, a, b, c, d, ok in zip(z['rows'], z['J0'], z['J_ref'], z['J_pg64'], Jh, agree):
        print('g17 %-9s row %2d  J(0) %10.3f  SLSQP %10.3f  projected gradient float64 %10.3f  MI355X %10.3f  %s'
              % (task, r, a, b, c, d, 'agrees' if ok else 'DISAGREES'))
    print('g17 %s: %d of %d rows disagree (reference alone: %d, float64 projected gradient: %d)'
          % (task, (~agree).sum(), B, (~z['ref_alone_ok']).sum(), (~z['pg64_ok']).sum()))
    assert 4 * int((~agree).sum()) <= B


def test_warm_start_and_other_weights():
    import torch
    z, model, mpc, obs0, ref = mpc_setup('straight')
    u, J, _ = mpc.solve(obs0, ref_indexes=ref, iterations=10)
    w = mpc.warm_start(u)
    u2, J2, info2 = mpc.solve(obs0, ref_indexes=ref, u_init=w, iterations=3)
    assert bool((J2 <= info2['J_history'][0]).all()) and float(u2.abs().max()) <= 1.0
    from env_build_amd.mpc import OpenLoopMPC
    other = OpenLoopMPC(model, horizon=5, weights=(-1.0, 0.0, 0.0, 0.0, 0.0), iterations=5)
    u3, J3, info3 = other.solve(obs0, ref_indexes=ref, check_every=2, tol=0.0)
    assert u3.shape[0] == 5 and bool((J3 <= info3['J_history'][0]).all())
    with pytest.raises(ValueError):
        mpc.solve(obs0)                                # training mode needs ref_indexes
    with pytest.raises(ValueError):
        OpenLoopMPC(model, horizon=100000)


def test_mpc_example_runs_a_few_control_steps():
    mod = load_example('mpc_open_loop')
    r = mod.run(n_env=128, control_steps=3, iterations=8)
    import torch
    assert torch.isfinite(r['J_first']).all() and bool((r['J_first'] <= r['J0_first']).all())
    assert bool((r['J_first'] < r['J0_first']).any()) and torch.isfinite(r['reward_sum']).all()
    assert r['launches'] == 3 * (1 + 8 * 4)
