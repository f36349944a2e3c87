"""CPU (-m "not gpu"): the candidate-tape gradient family on the host (the ABI of include/envbuild_cand_grad.h:
tests/test_family_abi.py): its kernel uses no scratch in any instantiation; the solver's start dimension
(env_build_amd/mpc.py: projected_gradient on [K, H, B, 2]) is K independent solves bit for bit on a non-convex toy cost; the G19
fixtures (scripts/gen_golden_mpc_paths.py) are well-formed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from env_build_amd import build as eb_build
from tests import _grad_cases
from tests._helpers import GOLDEN

TASKS = ('left', 'straight', 'right')


def test_the_kernel_uses_no_scratch_in_any_instantiation(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.isfile(hipcc) and not shutil.which(hipcc):
        pytest.skip('hipcc is not installed: the resource-usage remarks need the compiler')
    src = os.path.join(eb_build.CSRC, 'eb_rollout_tape_cand_vjp.hip')
    r = subprocess.run([hipcc] + eb_build.FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-c', src, '-o', str(tmp_path / 'cg.o')],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-2000:]
    names = re.findall(r'Function Name: (\S+)', r.stdout)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', r.stdout)]
    occupancy = [int(v) for v in re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', r.stdout)]
    kernels = [i for i, n in enumerate(names) if 'rollout_tape_cand_vjp_kernel' in n]
    assert len(kernels) == 6 and len(scratch) == len(names) == len(occupancy)      # 3 tasks x 2 record counts per lane
    for i in kernels:
        print('%s: scratch %d B, %d waves per SIMD' % (names[i], scratch[i], occupancy[i]))
        assert scratch[i] == 0, names[i]
        assert occupancy[i] >= 3, names[i]                                         # __launch_bounds__(256, 3)


# ---- the solver's start dimension, on the CPU ----
def toy_problem(dtype, seed=0, H=8, B=64):
    """tests/test_tape_cand_host.py:toy_problem with reductions counted from the end, so that u may carry a leading start dimension:
    J_b(u) = scale_b (1/2 sum c (u - m_b)^2 + sum_j A_j exp(-|u - p_j|^2 / s)): a quadratic bowl with bumps (non-convex), envs of very
    different curvature, and one env whose cost turns NaN after the first evaluation (every trial rejected)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    m = (torch.randn((H, B, 2), generator=g, dtype=torch.float64) * 1.5).to(dtype)
    c = (torch.rand((H, 1, 2), generator=g, dtype=torch.float64) * 20.0 + 0.05).to(dtype)
    scale = torch.logspace(-3, 2, B, dtype=torch.float64).to(dtype)
    bumps = [((torch.rand((H, B, 2), generator=g, dtype=torch.float64) * 2 - 1).to(dtype), amp) for amp in (30.0, -20.0, 45.0)]
    state = {'calls': 0}

    def value(u, need_grad):
        J = (0.5 * c * (u - m) ** 2).sum((-3, -1))
        grad = c * (u - m) if need_grad else None
        for p, amp in bumps:
            e = amp * torch.exp(-((u - p) ** 2).sum((-3, -1)) / 0.8)
            J = J + e
            if need_grad:
                grad = grad + e.unsqueeze(-1).unsqueeze(-3) * (-2.0 / 0.8) * (u - p)
        J = J * scale
        if need_grad:
            grad = grad * scale.view(1, -1, 1)
        return J, grad

    def evaluate(u, need_grad):
        state['calls'] += 1
        J, grad = value(u, need_grad)
        if state['calls'] > 1:
            J = J.clone()
            J[..., B - 1] = float('nan')
        return J, grad
    return evaluate, state


def starts_for(dtype, K, H=8, B=64):
    import torch
    g = torch.Generator().manual_seed(11)
    U = torch.rand((K, H, B, 2), generator=g, dtype=torch.float64) * 2.4 - 1.2      # some beyond the box: the solver clips
    U[0] = 0.0
    return U.to(dtype)


def same(a, b):            # torch.equal is False for NaN == NaN: the NaN env's cost is compared by position
    import torch
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_torch_reduces_a_slice_of_the_start_dimension_like_the_slice_alone():
    """what the bit claim below rests on: x.sum((1, 3))[k] == x[k].sum((0, 2)), and amax, on this machine's torch"""
    import torch
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.float64):
        for K in (1, 3, 4):
            for H in (8, 25):
                for B in (9, 64, 4096):
                    x = torch.randn((K, H, B, 2), generator=g, dtype=torch.float64).to(dtype)
                    for k in range(K):
                        assert torch.equal(x.sum((-3, -1))[k], x[k].sum((0, 2))) and torch.equal(x.abs().amax((-3, -1))[k], x[k].abs().amax((0, 2)))


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
@pytest.mark.parametrize('fused', [False, True])
def test_a_k_start_run_is_k_separate_runs_bit_for_bit(dtype_name, fused):
    import torch
    from env_build_amd.mpc import projected_gradient
    dtype = getattr(torch, dtype_name)
    K, iterations, trials = 3, 40, 3
    U0 = starts_for(dtype, K)

    def many_for(evaluate):
        def evaluate_many(UU):
            assert UU.shape[0] == trials and UU.is_contiguous()
            return torch.stack([evaluate(UU[t], False)[0] for t in range(trials)])
        return evaluate_many if fused else None
    evaluate, state = toy_problem(dtype)
    U, J, info = projected_gradient(evaluate, U0, iterations, ls_trials=trials, evaluate_many=many_for(evaluate))
    assert U.shape == (K, 8, 64, 2) and J.shape == (K, 64)
    hist, acc = info['J_history'], info['accepted']
    assert hist.shape == (iterations + 1, K, 64) and acc.shape == (iterations, K, 64) and acc.dtype == torch.bool
    assert info['iterations'] == iterations and info['evaluations'] == 1 + iterations * (trials + 1)
    assert info['launches_per_iteration'] == (2 if fused else trials + 1)
    assert state['calls'] == info['evaluations']                         # one call scores all K starts
    assert float(U.abs().max()) <= 1.0
    assert bool((hist[1:, :, :-1] <= hist[:-1, :, :-1]).all())            # per start: J never increases
    assert same(hist[-1], J)
    assert not acc[:, :, -1].any() and torch.equal(U[:, :, -1], U0.clamp(-1, 1)[:, :, -1])      # the NaN env keeps its iterate in every start
    assert bool(acc[:, :, :-1].any()) and bool((~acc[:, :, :-1]).any())   # accepted and rejected env-iterations both occur
    for k in range(K):                                                    # K separate [H, B, 2] runs
        evaluate, _ = toy_problem(dtype)
        u1, J1, i1 = projected_gradient(evaluate, U0[k], iterations, ls_trials=trials, evaluate_many=many_for(evaluate))
        assert torch.equal(u1, U[k]) and same(J1, J[k]), 'start %d' % k
        assert same(i1['J_history'], hist[:, k]) and torch.equal(i1['accepted'], acc[:, k])
    # the starts do end in different places: the cost is non-convex
    assert not torch.equal(torch.nan_to_num(J[0]), torch.nan_to_num(J[1]))
    # starts permuted along K: permuted u, J, J_history, accepted
    order = [2, 0, 1]
    evaluate, _ = toy_problem(dtype)
    Up, Jp, ip = projected_gradient(evaluate, U0[order].contiguous(), iterations, ls_trials=trials, evaluate_many=many_for(evaluate))
    assert torch.equal(Up, U[order]) and same(Jp, J[order]) and same(ip['J_history'], hist[:, order]) and torch.equal(ip['accepted'], acc[:, order])


# ---- G19 ----
@pytest.mark.parametrize('task', TASKS)
def test_g19_is_well_formed(task):
    path = os.path.join(GOLDEN, 'g19_mpc_paths_%s.npz' % task)
    assert os.path.getsize(path) <= 1 << 20
    z = np.load(path)
    B, H, P = len(z['rows']), int(z['horizon']), 3
    D = z['obs0'].shape[1]
    assert H == 25 and 8 <= B <= 16 and list(z['rows']) == sorted(set(z['rows'].tolist()))
    assert z['obs0'].shape == (B, D) and z['obs0'].dtype == np.float32 and z['obs_paths'].shape == (P, B, D)
    assert np.array_equal(np.delete(z['obs_paths'], [6, 7, 8], 2), np.broadcast_to(np.delete(z['obs0'].astype(np.float64), [6, 7, 8], 1), (P, B, D - 3)))
    for k in ('J0', 'J_ref', 'J_ref2', 'J_pg64'):
        assert z[k].shape == (P, B) and np.isfinite(z[k]).all(), k
    assert z['u_ref'].shape == (P, H, B, 2) and np.abs(z['u_ref']).max() <= 1.0 and np.abs(z['tape2']).max() <= 1.0
    assert (z['J_ref'] <= z['J0'] + 1e-9).all()                          # SLSQP from the zero tape does not end above it
    assert np.array_equal(z['Jbest_ref'], z['J_ref'].min(0))
    assert np.array_equal(z['ref_alone_ok'], z['J_ref2'].min(0) <= z['Jbest_ref'] + 0.1)
    assert 4 * int((~z['ref_alone_ok']).sum()) <= B                       # the cap the GPU test puts on the solver, met by the reference
    assert np.array_equal(z['weights'], np.array([-1, 10, 0, 0, 0], np.float32))
    for tag in ('0', '2'):
        assert z['g%s_act64' % tag].shape == (P, H, B, 2) and z['g%s_act32' % tag].shape == (P, H, B, 2)
        assert np.isfinite(z['g%s_act64' % tag]).all() and z['E%s_act' % tag].shape == (P, 2) and z['ok%s' % tag].shape == (P, B)
        assert (~z['ok%s' % tag]).sum() <= _grad_cases.MAX_EXCLUDED * z['ok%s' % tag].size
    kind = z['tape2_kind']
    assert kind.shape == (P, B) and set(np.unique(kind)) <= {0, 1, 2}
    for p in range(P):
        for b in range(B):
            want = (z['u_ref'][p, :, b], 0.5 * z['u_ref'][p, :, b], 0.0 * z['u_ref'][p, :, b])[kind[p, b]]
            assert np.array_equal(z['tape2'][p, :, b], want)
    assert np.array_equal(z['t0'], np.array([0, 5, 10, 15])[z['rows'] // 32]) and np.array_equal(z['g5_row'], z['rows'] % 32)
