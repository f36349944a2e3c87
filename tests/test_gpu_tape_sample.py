"""GPU (-m gpu): eb_rollout_tape_sample — S perturbed action tapes per env drawn, rolled out, scored and averaged in one launch
(include/envbuild_sample.h, csrc/eb_rollout_tape_sample.hip).

Exact: samples_out is sample.sample_tapes_reference bit for bit; cost is eb_rollout_tape_cand's cost over the dumped tapes bit for
bit (chunked by its limit); best_index is mpc.first_minimum(cost), best_cost / best_tape that sample's bits; permutation, slicing,
repetition.  Bounded: mean_tape is within (S + 16) * 2^-24 absolute of the float64 soft-min average formed from the returned cost
and samples_out — the bound of an S-term fp32 sum of products bounded by 1 with weights good to a few ulp.

The NaN case.  A NaN cost on one env must leave the other envs alone.  No NOMINAL yields a NaN cost: the action transform
clips with fmin / fmax (DAM:120 as eb_device.h:action_transform restates it), which maps a NaN action to the bound, so the cost of a
NaN tape is finite.  test_a_nan_env_leaves_the_others_alone therefore runs both: a NaN NOMINAL (the env's samples carry the NaN,
its costs stay finite, the other envs' bits are unchanged) and a NaN ROW of obs0 (every cost of that env is NaN: index 0, the other
envs' bits unchanged)."""
import ctypes as C

import numpy as np
import pytest

from env_build_amd import _capi
from tests._helpers import golden
from tests._grad_cases import TASKS
from tests._tape import G5, NATIVE, WEIGHTS, SampleModel, bits, edge_synthetic_case, load_example, mpc_setup, same, synthetic_case

pytestmark = pytest.mark.gpu


def mean_bound(S):
    return (S + 16) * 2.0 ** -24


def check_launch(m, obs0, nominal, ri, pid, S, what, seed=3, counter=5, sigma=(0.3, 0.25), beta=0.0, inv_lambda=0.5, w5=WEIGHTS[0],
                 env_ids=None):
    """one launch with every output, held to everything the header states -> its outputs"""
    import torch
    from env_build_amd.mpc import first_minimum
    from env_build_amd.sample import sample_tapes_reference, softmin_mean_reference
    H, n = nominal.shape[0], obs0.shape[0]
    out = m.t_sample(obs0, nominal, S, ri, pid, env_ids, seed, counter, sigma, beta, inv_lambda, w5)
    want = sample_tapes_reference(nominal.cpu(), S, seed, counter, sigma, beta, None if env_ids is None else env_ids.cpu())
    assert same(out['samples'].cpu(), want), '%s: samples_out differs from the restatement in %d of %d words' % (
        what, int((bits(out['samples'].cpu()) != bits(want)).sum()), want.numel())
    cost = m.cand_cost(obs0, out['samples'], ri, pid, w5)
    assert same(out['cost'], cost), '%s: cost differs from eb_rollout_tape_cand in %d of %d words' % (
        what, int((bits(out['cost']) != bits(cost)).sum()), cost.numel())
    idx = first_minimum(cost)
    assert torch.equal(out['best_index'].long(), idx), what
    assert same(out['best_cost'], cost.gather(0, idx.view(1, n))[0]), what
    assert same(out['best_tape'], out['samples'].gather(0, idx.view(1, 1, n, 1).expand(1, H, n, 2))[0]), what
    lam = float('inf') if inv_lambda == 0 else 1.0 / inv_lambda
    mean64, _ = softmin_mean_reference(out['samples'].double(), out['cost'].double(), lam)
    err = float((out['mean_tape'].double() - mean64).abs().max())
    assert err <= mean_bound(S), '%s: mean_tape is %.3e from the float64 soft-min average, bound %.3e' % (what, err, mean_bound(S))
    assert float(out['mean_tape'].abs().max()) <= 1.0
    if not any(w5):
        assert not bool(out['cost'].any()) and not bool(torch.signbit(out['cost']).any())       # all weights zero: +0
    return out


def box_nominal(tape):
    """the synthetic tape (a few actions beyond +-1.05) with entries exactly on the box"""
    nominal = tape.clone()
    nominal[0, 0, 0] = 1.0
    nominal[-1, -1, 1] = -1.0
    return nominal


S_GRID = (1, 2, 63, 64, 65, 128, 129, 256, 257, 1024)      # the wave, block and round boundaries


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_shape_grid(task, mode):
    """S over the wave, block and round boundaries, n_env in {1, 3, 5} (an idle env slot in the last block at S = 64 and 128; S = 1024
    at n_env = 2), H in {1, 5, 25}, n_veh in {native, 16, 64}, n_future in {0, 2} — NOT their full product: two rotations of the
    other factors against S.  Every S runs twice in every (task, mode); over the six (task, mode) pairs every S meets every n_veh,
    every H and both n_future, but not every triple.  beta, the weights (zeros in different rows, all zero), a zero sigma component
    and explicit env ids rotate with them."""
    import torch
    base = TASKS.index(task) * 2 + (mode == 'selecting')
    models = {}
    n = 0
    for i, S in [(i + 4 * r, S) for r in (0, 1) for i, S in enumerate(S_GRID)]:      # the second rotation: every factor shifted
        k = base + i
        n_veh, nf = (NATIVE[task], 16, 64)[k % 3], (0, 2)[(k // 3) % 2]
        H, B = (1, 5, 25)[(k + i // 3) % 3], 2 if S == 1024 else (1, 3, 5)[(k // 2) % 3]
        if (n_veh, nf) not in models:
            models[(n_veh, nf)] = SampleModel(task, n_veh=n_veh, n_future=nf, mode=mode)
        m = models[(n_veh, nf)]
        assert m.sample_max(25) >= 1024 and m.sample_max(128) >= 1024
        obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, task, B, H, seed=100 * S + k)
        ids = torch.tensor([7, 0, 123456, 2 ** 31 - 1, 3][:B], dtype=torch.int32, device='cuda') if k % 2 else None
        sigma = ((0.3, 0.25), (0.4, 0.0), (0.0, 0.5))[k % 3]
        check_launch(m, obs0, box_nominal(tape), ri, pid, S, '%s %s S%d B%d H%d N%d nf%d' % (task, mode, S, B, H, n_veh, nf),
                     sigma=sigma, beta=(0.0, 0.7)[k % 2], inv_lambda=(0.5, 0.05, 2.0)[k % 3], w5=WEIGHTS[k % len(WEIGHTS)], env_ids=ids)
        n += 1
    assert n == 2 * len(S_GRID)


@pytest.mark.parametrize('task', TASKS)
def test_crowded_remote_and_near_wall_scenes(task):
    """every vehicle within 4.5 m of its ego, a third of the egos off the closest-point cell grid, a third on the lane's walls, ids out
    of range (edge_synthetic_case), at 32 and 64 slots: four, two and one env per block, and two rounds"""
    for n_veh, mode in ((32, 'training'), (64, 'selecting')):
        m = SampleModel(task, n_veh=n_veh, n_future=0, mode=mode)
        for S, B, H in ((64, 7, 25), (100, 41, 5), (257, 6, 5)):
            obs0, tape, ri, pid, _g, _g5 = edge_synthetic_case(m, task, max(B, 120), H, seed=n_veh + S)   # (the helper wants its far egos)
            obs0, tape, ri = obs0[:B].contiguous(), tape[:, :B].contiguous(), None if ri is None else ri[:B].contiguous()
            out = check_launch(m, obs0, tape, ri, pid, S, 'edge %s N%d S%d' % (task, n_veh, S), beta=0.7, w5=WEIGHTS[3])
            assert bool((out['cost'] > 0).all())


@pytest.mark.parametrize('name', G5)
def test_reference_start_rows(name):
    """the start rows of every g5 fixture (the reference's own scenes), the fixture's tape as the nominal"""
    _, _, task, N, mode, nf = name.split('_')
    g = golden(name)
    m = SampleModel(task, n_veh=int(N[1:]), n_future=int(nf[2:]), mode=mode, modes=[str(v) for v in g['modes']])
    rows = slice(0, 24)
    obs0, tape = m.to_dev(g['obs0'][rows]), m.to_dev(np.ascontiguousarray(g['actions'][:, rows]))
    ri = m.to_dev(g['ref_idx'][rows], np.int32) if mode == 'training' else None
    assert len(G5) >= 6
    check_launch(m, obs0, tape, ri, 1, 96, name, beta=0.7)


def test_softmin_limits():
    """inv_lambda = 0 is the plain average; a large inv_lambda gives best_tape, both within the bound"""
    m = SampleModel('left', n_veh=16, n_future=0, mode='training')
    S, B, H = 129, 5, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=12)
    flat = check_launch(m, obs0, tape, ri, pid, S, 'plain average', inv_lambda=0.0)
    err = float((flat['mean_tape'].double() - flat['samples'].double().mean(0)).abs().max())
    assert err <= mean_bound(S)
    sharp = check_launch(m, obs0, tape, ri, pid, S, 'sharp', inv_lambda=1e9)
    assert float((sharp['mean_tape'] - sharp['best_tape']).abs().max()) <= mean_bound(S)
    assert same(sharp['cost'], flat['cost']) and same(sharp['best_tape'], flat['best_tape'])


def test_a_nan_env_leaves_the_others_alone():
    """see the module's docstring: a NaN nominal (finite costs: the action clip maps NaN to the bound) and a NaN row (all costs NaN:
    index 0, best_cost NaN, the mean is sample 0); the other envs' bits are unchanged in both"""
    import torch
    m = SampleModel('straight', n_veh=16, n_future=0, mode='training')
    S, B, H = 65, 3, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'straight', B, H, seed=4)
    clean = m.t_sample(obs0, tape, S, ri, pid, beta=0.7)
    keep = [0, 2]

    def others_unchanged(out):
        for k in ('cost', 'best_cost', 'best_index'):
            assert same(out[k][..., keep], clean[k][..., keep]), k
        for k in ('best_tape', 'mean_tape', 'samples'):
            assert same(out[k][..., keep, :], clean[k][..., keep, :]), k
    nominal = tape.clone()
    nominal[3, 1, 0] = float('nan')
    a = m.t_sample(obs0, nominal, S, ri, pid, beta=0.7)
    others_unchanged(a)
    assert bool(torch.isnan(a['samples'][:, 3, 1, 0]).all()) and bool(torch.isfinite(a['cost']).all())
    assert same(a['cost'], m.cand_cost(obs0, a['samples'], ri, pid, WEIGHTS[0]))
    rows = obs0.clone()
    rows[1, 3] = float('nan')
    b = m.t_sample(rows, tape, S, ri, pid, beta=0.7)
    others_unchanged(b)
    assert bool(torch.isnan(b['cost'][:, 1]).all()) and int(b['best_index'][1]) == 0 and bool(torch.isnan(b['best_cost'][1]))
    assert same(b['best_tape'][:, 1], b['samples'][0, :, 1]) and same(b['mean_tape'][:, 1], b['samples'][0, :, 1])
    assert same(b['samples'], clean['samples'])


def test_a_tape_pointer_aligned_to_four_bytes_only():
    """nominal (and every output tape) at an odd float offset of its buffer: the bits of the aligned launch"""
    import torch
    m = SampleModel('left', n_veh=16, n_future=0, mode='training')
    S, B, H = 65, 3, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=6)
    full = m.t_sample(obs0, tape, S, ri, pid, beta=0.7)
    odd = torch.empty(tape.numel() + 1, device='cuda')[1:].view(H, B, 2)
    odd.copy_(tape)
    assert odd.is_contiguous() and odd.data_ptr() % 8 == 4
    got = m.t_sample(obs0, odd, S, ri, pid, beta=0.7)
    for k in full:
        assert same(got[k], full[k]), k


def test_independence():
    """a permuted batch with permuted env ids gives permuted bits, a slice the slice; two launches repeat their bits; another counter
    changes every sample but sample 0; any subset of the outputs has the bits of the full set"""
    import torch
    m = SampleModel('right', n_veh=16, n_future=2, mode='training')
    for S, B in ((64, 13), (128, 7), (300, 4)):
        H = 5
        obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'right', B, H, seed=3 + S)
        ids = torch.arange(B, dtype=torch.int32, device='cuda') * 5 + 2
        kw = dict(seed=8, counter=2, beta=0.7, w5=WEIGHTS[3])
        full = m.t_sample(obs0, tape, S, ri, pid, ids, **kw)
        again = m.t_sample(obs0, tape, S, ri, pid, ids, **kw)
        for k in full:
            assert same(full[k], again[k]), k
        perm = torch.randperm(B, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
        p = m.t_sample(obs0[perm].contiguous(), tape[:, perm].contiguous(), S, ri[perm].contiguous(), pid, ids[perm].contiguous(), **kw)
        for k in ('cost', 'best_cost', 'best_index'):
            assert same(p[k], full[k][..., perm]), 'permuted %s S%d' % (k, S)
        for k in ('best_tape', 'mean_tape', 'samples'):
            assert same(p[k], full[k][..., perm, :]), 'permuted %s S%d' % (k, S)
        for first, n in ((0, 1), (B - 1, 1), (1, 3)):
            s = slice(first, first + n)
            q = m.t_sample(obs0[s].contiguous(), tape[:, s].contiguous(), S, ri[s].contiguous(), pid, ids[s].contiguous(), **kw)
            for k in ('cost', 'best_cost', 'best_index'):
                assert same(q[k], full[k][..., s]), 'slice %d+%d %s S%d' % (first, n, k, S)
            for k in ('best_tape', 'mean_tape', 'samples'):
                assert same(q[k], full[k][..., s, :]), 'slice %d+%d %s S%d' % (first, n, k, S)
        other = m.t_sample(obs0, tape, S, ri, pid, ids, seed=8, counter=3, beta=0.7, w5=WEIGHTS[3])
        assert same(other['samples'][0], full['samples'][0]) and same(other['cost'][0], full['cost'][0])
        free = (other['samples'][1:].abs() < 1.0) & (full['samples'][1:].abs() < 1.0)
        assert bool((other['samples'][1:] != full['samples'][1:])[free].all()) and int(free.sum()) > free.numel() // 3
        for want in (('cost',), ('mean_tape',), ('best_tape',), ('best_index', 'best_cost'), ('samples',)):
            part = m.t_sample(obs0, tape, S, ri, pid, ids, want=want, **kw)
            for k in want:
                assert same(part[k], full[k]), 'subset %s S%d' % (k, S)


def test_one_medium_run_every_cost():
    """4096 x 16 x 25, S = 64: every cost against the chunked candidate path over the dumped tapes; the reduction against torch"""
    import torch
    from env_build_amd.mpc import first_minimum
    m = SampleModel('left', n_veh=16, n_future=0, mode='training')
    S, B, H = 64, 4096, 25
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=7)
    out = m.t_sample(obs0, tape, S, ri, pid, seed=1, counter=9, sigma=(0.4, 0.4), beta=0.7, inv_lambda=0.2)
    cost = m.cand_cost(obs0, out['samples'], ri, pid, WEIGHTS[0])
    assert same(out['cost'], cost), 'cost differs in %d of %d words' % (int((bits(out['cost']) != bits(cost)).sum()), cost.numel())
    idx = first_minimum(cost)
    assert torch.equal(out['best_index'].long(), idx) and same(out['best_cost'], cost.gather(0, idx.view(1, B))[0])
    assert same(out['best_tape'], out['samples'].gather(0, idx.view(1, 1, B, 1).expand(1, H, B, 2))[0])
    assert len(set(idx.tolist())) > S // 2 and bool(torch.isfinite(out['mean_tape']).all())


def test_refusals():
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.sample import rollout_tape_samples, tape_sample_max
    m = SampleModel('left', n_veh=64, n_future=0, mode='training')
    limit = m.sample_max()
    assert limit >= 1024
    B, H = 4, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=1)
    ok = dict(ri=ri, path_id=pid)
    m.t_sample(obs0, tape, 8, **ok)
    with pytest.raises(ValueError) as e:                                   # over the limit: the limit in the message
        m.t_sample(obs0, tape, limit + 1, want=('best_cost',), **ok)
    assert str(limit) in str(e.value) and 'samples' in str(e.value)
    bad = [dict(want=()),                                                  # every output NULL
           dict(w5=None), dict(sigma=None), dict(sigma=(-0.1, 0.2)), dict(sigma=(0.1, float('nan'))),
           dict(beta=1.0), dict(beta=-0.1), dict(beta=float('nan')),
           dict(inv_lambda=-1.0), dict(inv_lambda=float('inf')), dict(inv_lambda=float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            m.t_sample(obs0, tape, 8, **dict(ok, **kw))
    with pytest.raises(ValueError):                                        # horizon beyond 128
        m.t_sample(obs0, torch.zeros((129, B, 2), device='cuda'), 8, **ok)
    with pytest.raises(ValueError) as e:                                   # training mode without ref_idx
        m.t_sample(obs0, tape, 8, None, pid)
    assert 'ref_idx' in str(e.value)
    sel = SampleModel('left', n_veh=8, n_future=0, mode='selecting')
    o8, t8, _ri, _pid, _g, _g5 = synthetic_case(sel, 'left', B, H, seed=2)
    for p in (3, -1):
        with pytest.raises(ValueError):                                    # a path id out of range in selecting mode
            sel.t_sample(o8, t8, 8, None, p)
    # n_env == 0 and n_samples == 0: no-ops that succeed
    z = (C.c_float * 2)(0.1, 0.1)
    m.api.rollout_tape_sample(m.h, 0, 8, 5, None, None, None, 0, None, 0, 0, z, 0.0, 1.0, None, None, None, None, None, None, None, m.stream)
    m.api.rollout_tape_sample(m.h, 4, 0, 5, None, None, None, 0, None, 0, 0, z, 0.0, 1.0, None, None, None, None, None, None, None, m.stream)
    # the facade: one launch, the raw entry's bits
    model = EnvironmentModel('left', 0, mode='training', n_veh=64)
    assert tape_sample_max(model, H) == limit
    out = rollout_tape_samples(model, obs0, tape, 70, seed=3, counter=4, sigma=(0.3, 0.2), beta=0.5, lam=2.0, ref_indexes=ri, dump_samples=True)
    raw = m.t_sample(obs0, tape, 70, ri, pid, None, 3, 4, (0.3, 0.2), 0.5, 0.5, WEIGHTS[0])
    for k in ('cost', 'best_tape', 'best_cost', 'best_index', 'mean_tape', 'samples'):
        assert same(out[k], raw[k]), k
    assert sorted(rollout_tape_samples(model, obs0, tape, 8, 0, 0, (0.1, 0.1), ref_indexes=ri, want=('best',))) == ['best_cost', 'best_index', 'best_tape']
    with pytest.raises(_capi.EbError):                                     # fp16 state has no sampled form
        rollout_tape_samples(EnvironmentModel('left', 0, mode='training', state_dtype='float16'), obs0, tape, 8, 0, 0, (0.1, 0.1))
    with pytest.raises(ValueError):
        rollout_tape_samples(model, obs0, tape, 8, 0, 0, (0.1, 0.1), lam=0.0, ref_indexes=ri)


# ---- the solver ----
@pytest.mark.parametrize('task', TASKS)
def test_sampling_mpc_on_the_g17_start_states(task):
    """J_history never increases; J <= J of the initial nominal (both by the same independent evaluation); u in the box;
    launches == iterations + 1; a second solve with the same seed repeats its bits.  The share of rows that agree with the reference
    optimiser under the J <= J_ref + 0.1 rule is printed, not asserted (DESIGN.md §13 records it)."""
    import torch
    from env_build_amd.mpc import SamplingMPC
    z, model, mpc, obs0, ref = mpc_setup(task)
    H, B = int(z['horizon']), obs0.shape[0]
    smpc = SamplingMPC(model, horizon=H, seed=1)
    u, J, info = smpc.solve(obs0, ref_indexes=ref)
    hist = info['J_history']
    assert u.shape == (H, B, 2) and float(u.abs().max()) <= 1.0 and bool(torch.isfinite(J).all())
    assert hist.shape == (smpc.iterations + 1, B) and bool((hist[1:] <= hist[:-1]).all()) and same(hist[-1], info['J_kernel'])
    assert info['launches'] == smpc.iterations + 1 and info['counter_next'] == smpc.iterations
    J_init = mpc.value_and_grad(obs0, torch.zeros_like(u), ref, 0, need_grad=False)[0]
    assert bool((J <= J_init).all()) and bool((J < J_init).any())
    assert same(J, mpc.value_and_grad(obs0, u, ref, 0, need_grad=False)[0])
    assert float((J - info['J_kernel']).abs().max()) <= 1e-5 * float(J.abs().max()) + 1e-5    # two summation orders of one cost
    u2, J2, info2 = smpc.solve(obs0, ref_indexes=ref)
    assert same(u2, u) and same(J2, J) and same(info2['J_history'], hist)
    u3, _J3, _ = smpc.solve(obs0, ref_indexes=ref, counter=info['counter_next'])
    assert not same(u3, u)
    agree = J.double().cpu().numpy() <= z['J_ref'] + 0.1
    print('g17 %s SamplingMPC alone (defaults: S %d, %d iterations): %d of %d rows disagree with J_ref + 0.1; mean J %.3f (J_ref %.3f)'
          % (task, smpc.n_samples, smpc.iterations, int((~agree).sum()), B, float(J.mean()), float(z['J_ref'].mean())))


@pytest.mark.parametrize('task', TASKS)
def test_hybrid_never_ends_above_the_default_solver(task):
    """polish: the zero tape and the sampled tape both descend; start 0's descent is the default solver's, so J <= J_default on EVERY
    row, hence no more rows disagree with J_ref than the default solver's (at most one quarter, tests/test_gpu_mpc.py)"""
    import torch
    from env_build_amd.mpc import OpenLoopMPC, SamplingMPC
    z, model, mpc, obs0, ref = mpc_setup(task)
    H, B = int(z['horizon']), obs0.shape[0]
    u_d, J_default, info_d = mpc.solve(obs0, ref_indexes=ref)
    hybrid = SamplingMPC(model, horizon=H, seed=1, polish=OpenLoopMPC(model, horizon=H))
    u, J, info = hybrid.solve(obs0, ref_indexes=ref)
    for b in range(B):
        print('g17 %-9s row %2d  default %10.3f  sampled %10.3f  hybrid %10.3f  SLSQP %10.3f'
              % (task, b, float(J_default[b]), float(info['J_sampled'][b]), float(J[b]), float(z['J_ref'][b])))
    assert float(u.abs().max()) <= 1.0 and bool(torch.isfinite(J).all())
    assert same(info['polish']['J_starts'][0], J_default), 'start 0 of the polish is not the default solver bit for bit'
    assert bool((J <= J_default).all())
    assert info['launches'] == hybrid.iterations + 1 + info['polish']['launches']
    disagree = int((J.double().cpu().numpy() > z['J_ref'] + 0.1).sum())
    default = int((J_default.double().cpu().numpy() > z['J_ref'] + 0.1).sum())
    print('g17 %s hybrid: %d of %d rows disagree (default solver: %d); %d rows end below the default solver'
          % (task, disagree, B, default, int((J < J_default).sum())))
    assert disagree <= default and 4 * disagree <= B
    with pytest.raises(ValueError):
        SamplingMPC(model, horizon=H, polish=OpenLoopMPC(model, horizon=H - 1))


def test_sampling_example_runs_a_few_control_steps():
    import torch
    mod = load_example('mpc_sampling')
    r = mod.run(n_env=128, control_steps=3, iterations=4, n_samples=128)
    assert torch.isfinite(r['J_first']).all() and torch.isfinite(r['reward_sum']).all() and torch.isfinite(r['J_last']).all()
    slack = 1e-5 * r['J0_first'].abs() + 1e-5              # J0 is the kernel's sum, J the independent evaluation's
    assert bool((r['J_first'] <= r['J0_first'] + slack).all()) and bool((r['J_first'] < r['J0_first']).any())
    assert r['launches'] == 3 * (4 + 1)
    p = mod.run(n_env=64, control_steps=2, iterations=3, n_samples=64, polish=True, polish_iterations=4)
    assert torch.isfinite(p['J_last']).all() and p['launches'] > 2 * (3 + 1)
