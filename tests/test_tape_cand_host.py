"""CPU (-m "not gpu"): the candidate-tape family on the host (the ABI of include/envbuild_cand.h: tests/test_family_abi.py): the solver's
fused line search (env_build_amd/mpc.py:
projected_gradient with evaluate_many) reproduces the sequential one bit for bit on a non-convex toy cost; the K-start selection
rule (mpc.best_start) picks the first minimum and never a NaN."""
import pytest


# ---- the solver's fused line search, on the CPU ----
def toy_problem(dtype, seed=0, H=8, B=64):
    """J_b(u) = scale_b (1/2 sum c (u - m_b)^2 + sum_j A_j exp(-|u - p_j|^2 / s)): a quadratic bowl with bumps (non-convex), envs of
    very different curvature, and one env whose cost turns NaN after the first evaluation (every trial rejected)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    m = (torch.randn((H, B, 2), generator=g, dtype=torch.float64) * 1.5).to(dtype)
    c = (torch.rand((H, 1, 2), generator=g, dtype=torch.float64) * 20.0 + 0.05).to(dtype)
    scale = torch.logspace(-3, 2, B, dtype=torch.float64).to(dtype)
    bumps = [((torch.rand((H, B, 2), generator=g, dtype=torch.float64) * 2 - 1).to(dtype), amp) for amp in (30.0, -20.0, 45.0)]
    state = {'calls': 0}

    def value(u, need_grad):
        J = (0.5 * c * (u - m) ** 2).sum((0, 2))
        grad = c * (u - m) if need_grad else None
        for p, amp in bumps:
            e = amp * torch.exp(-((u - p) ** 2).sum((0, 2)) / 0.8)
            J = J + e
            if need_grad:
                grad = grad + e.view(1, -1, 1) * (-2.0 / 0.8) * (u - p)
        J = J * scale
        if need_grad:
            grad = grad * scale.view(1, -1, 1)
        return J, grad

    def evaluate(u, need_grad):
        state['calls'] += 1
        J, grad = value(u, need_grad)
        if state['calls'] > 1:
            J = J.clone()
            J[B - 1] = float('nan')
        return J, grad
    return evaluate, torch.zeros((H, B, 2), dtype=dtype), state


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
@pytest.mark.parametrize('shrink', [0.25, 0.3])
def test_fused_line_search_has_the_bits_of_the_sequential_one(dtype_name, shrink):
    import torch
    from env_build_amd.mpc import projected_gradient
    dtype = getattr(torch, dtype_name)
    iterations, trials = 40, 3
    evaluate, u0, _ = toy_problem(dtype)
    u_a, J_a, info_a = projected_gradient(evaluate, u0, iterations, ls_trials=trials, shrink=shrink)
    evaluate, u0, state = toy_problem(dtype)
    seen = []

    def evaluate_many(U):
        assert U.shape == (trials,) + u0.shape and U.is_contiguous()
        J = torch.stack([evaluate(U[k], False)[0] for k in range(U.shape[0])])
        seen.append(J)
        return J
    u_b, J_b, info_b = projected_gradient(evaluate, u0, iterations, ls_trials=trials, shrink=shrink, evaluate_many=evaluate_many)

    def same(a, b):            # torch.equal is False for NaN == NaN: the NaN env's cost is compared by position
        return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    assert torch.equal(u_a, u_b) and same(J_a, J_b)
    assert same(info_a['J_history'], info_b['J_history']) and torch.equal(info_a['accepted'], info_b['accepted'])
    assert len(seen) == iterations and info_b['iterations'] == info_a['iterations'] == iterations
    assert info_a['launches_per_iteration'] == trials + 1 and info_b['launches_per_iteration'] == 2
    assert info_a['evaluations'] == info_b['evaluations'] == 1 + iterations * (trials + 1)
    # both selection paths are exercised: a trial later than the first is accepted somewhere, and some env-iteration is rejected
    acc, hist = info_b['accepted'], info_b['J_history']
    later = 0
    for it in range(iterations):
        J0, Jn = seen[it][0], hist[it + 1]
        took_later = torch.zeros_like(acc[it])
        for k in range(1, trials):
            took_later |= Jn == seen[it][k]
        later += int((acc[it] & (Jn != J0) & took_later).sum())
    rejected = int((~acc[:, :-1]).sum())
    print('fused line search %s shrink %g: %d env-iterations accepted at a later trial, %d rejected (NaN env aside) of %d'
          % (dtype_name, shrink, later, rejected, acc[:, :-1].numel()))
    assert later >= 1 and rejected >= 1
    assert not acc[:, -1].any() and not u_b[:, -1].any()                  # the NaN env keeps its iterate
    assert bool((hist[1:, :-1] <= hist[:-1, :-1]).all())


def test_best_start_takes_the_first_minimum_and_never_a_nan():
    import torch
    from env_build_amd.mpc import best_start, first_minimum
    nan = float('nan')
    J = torch.tensor([[3.0, 1.0, nan, nan, 2.0, nan],
                      [1.0, 1.0, 5.0, nan, nan, nan],
                      [1.0, 0.5, 4.0, nan, 2.0, 7.0]])
    want = torch.tensor([1, 2, 2, 0, 0, 2])           # first minimum; NaN never wins; all NaN -> start 0
    assert torch.equal(first_minimum(J), want)
    K, H, B = 3, 4, 6
    U = torch.arange(K * H * B * 2, dtype=torch.float32).reshape(K, H, B, 2) / (K * H * B * 2) * 3.0 - 1.5
    calls = []

    def fake(Uc):
        calls.append(Uc)
        return J
    u, idx, J_out = best_start(U, fake)
    assert len(calls) == 1 and torch.equal(calls[0], U.clamp(-1, 1))     # one call, on the clipped starts
    assert torch.equal(idx, want) and J_out is J
    for b in range(B):
        assert torch.equal(u[:, b], U.clamp(-1, 1)[int(want[b]), :, b])
    assert u.shape == (H, B, 2) and u.is_contiguous()
