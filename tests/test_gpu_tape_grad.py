"""GPU (-m gpu): eb_rollout_tape_vjp — value and gradient of an open-loop rollout in one launch (include/envbuild_grad.h,
csrc/eb_rollout_tape_vjp.hip) — against the G16 chain fixtures and the G18 edge chains (bound: tests/_grad_cases.py), bit for bit against the composed path
(eb_rollout_step launches that keep every pre-step obs, then eb_rollout_chain_vjp) and against eb_rollout_tape's forward, its
invariants, its refusals, and grad.rollout_tape against a loop of grad.rollout_step under torch.autograd."""
import numpy as np
import pytest

from env_build_amd import _capi
from tests._grad_cases import TASKS, MAX_EXCLUDED, cases, check_columns, check_zero_distance, edge_cases, zero_distance_case
from tests._tape import NATIVE, TapeModel, all_same, edge_synthetic_case, same, synthetic_case

pytestmark = pytest.mark.gpu


def model_for(task, c):
    return TapeModel(task, n_veh=c.n_veh, n_future=c.n_future, mode=c.mode)


def tape_meets_the_reference(task, cs, tag):
    rows = excluded = 0
    for c in cs:
        m = model_for(task, c)
        ri = None if c.ref_idx() is None else m.to_dev(c.ref_idx(), np.int32)
        o5, _oo, g0, gt = m.t_tape_vjp(m.to_dev(c['obs0']), m.to_dev(c['tape']), ri, c.path_id, m.to_dev(c['g_obs_final']), m.to_dev(c['g_out5_steps']))
        out5, g0, gt = o5.cpu().numpy(), g0.cpu().numpy(), gt.cpu().numpy()
        want = c['out5_f32'].astype(np.float64)
        ok = c['ok'] & (np.abs(out5 - want) <= 5e-6 + 1e-5 * np.abs(want)).all((0, 1))
        rows += len(ok); excluded += int((~ok).sum())
        check_columns(g0, c['g_obs64'], c['E_obs'], ok, '%s tape %s %s obs0' % (tag, task, c.name))
        check_columns(np.moveaxis(gt, 0, 1), np.moveaxis(c['g_act64'], 0, 1), c['E_act'], ok, '%s tape %s %s tape' % (tag, task, c.name))
    print('%s tape %s: %d of %d rows excluded' % (tag, task, excluded, rows))
    assert excluded <= MAX_EXCLUDED * rows


@pytest.mark.parametrize('task', TASKS)
def test_tape_vjp_meets_the_reference_gradients_and_forward(task):
    """g16: every chain case.  Gradients: |g - g64| <= 4 E_c + 2^-20 max|g64| per column over the flagged rows.  Forward: out5_steps
    against the fixtures' float32 forward as tests/test_gpu_grad.py holds it (rtol 1e-5 next to atol 5e-6; a row beyond it counts as
    excluded, under the same 1 % cap)."""
    tape_meets_the_reference(task, cases('g16_grad_chain', task), 'g16')


@pytest.mark.parametrize('task', TASKS)
def test_tape_vjp_meets_the_edge_chains(task):
    """g18: the chains that start on the junction's exit side and next to the entry lane's walls, held as the g16 chains are"""
    tape_meets_the_reference(task, edge_cases(task)[1], 'g18')


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_tape_vjp_has_the_bits_of_the_composed_path_in_crowded_remote_and_near_wall_scenes(task, mode):
    """32 and 64 slots, every record near, in every tile shape the launch picks by batch size (csrc/eb_rollout_tape_vjp.hip:
    tv_pick_tile — 32 envs per block from 2 * CUs blocks of 32 on, 16 from 2 * CUs blocks of 16 on, 8 below; 64 slots: 16 and 8), each
    batch leaving idle env lanes in its last block: the bits of the composed path and of eb_rollout_tape's forward."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 0
    for n_veh, tiles in ((32, (32, 16, 8)), (64, (16, 8))):
        m = TapeModel(task, n_veh=n_veh, n_future=0, mode=mode)
        for E in tiles:
            B = 2 * n_cu * E + 11 if E > 8 else 211
            H = 5 if E > 8 else 25
            obs0, tape, ri, pid, g_final, g5 = edge_synthetic_case(m, task, B, H, seed=1000 * n_veh + E)
            got = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5)
            want = m.t_composed(obs0, tape, ri, pid, g_final, g5)
            what = '%s %s N%d E%d B%d H%d' % (task, mode, n_veh, E, B, H)
            all_same(got, want, what)
            f5, fo = m.t_forward_tape(obs0, tape, ri, pid)
            assert same(got[0], f5) and same(got[1], fo), what + ': forward differs from eb_rollout_tape'
            assert bool(torch.isfinite(got[2]).all()) and bool(torch.isfinite(got[3]).all()), what
            assert bool((got[0][0, 3] > 0).all()), what       # every row has circle pairs below 2.5 m at the first step
            n += 1
    assert n == 5


@pytest.mark.parametrize('task', TASKS)
def test_zero_circle_distance_is_finite_and_the_same_in_both_kernels(task):
    """A vehicle whose circle centres coincide with the ego's (distance exactly 0: NaN in the reference, a contribution of 0 here):
    finite, the closed form of tests/_grad_cases.py:zero_distance_case within the case's column tolerance, and the same bits from
    eb_rollout_step_vjp and from a one-step eb_rollout_tape_vjp."""
    c, rows, obs, want = zero_distance_case(task)
    m = model_for(task, c)
    ri = None if c.ref_idx() is None else m.to_dev(c.ref_idx(), np.int32)
    ob, ac, g, g5 = m.to_dev(obs), m.to_dev(c['actions']), m.to_dev(c['g_obs_out']), m.to_dev(c['g_out5'])
    gi, ga = m.t_step_vjp(ob, ac, ri, c.path_id, g, g5)
    _o5, _oo, g0, gt = m.t_tape_vjp(ob, ac[None].contiguous(), ri, c.path_id, g, g5[None].contiguous())
    assert same(gi, g0) and same(ga, gt[0])
    check_zero_distance(c, rows, gi.cpu().numpy(), ga.cpu().numpy(), want, 'g18 %s zero distance' % task)


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_tape_vjp_has_the_bits_of_the_composed_path(task, mode):
    """n_veh in {native, 16, 32, 64} x H in {1, 5, 25} x n_future in {0, 2}: g_obs0, g_action_tape, out5_steps and obs_out equal the
    composed path's bit for bit; out5_steps and obs_out equal eb_rollout_tape's."""
    n = 0
    for n_veh in (NATIVE[task], 16, 32, 64):
        for nf in (0, 2):
            m = TapeModel(task, n_veh=n_veh, n_future=nf, mode=mode)
            assert m.max_horizon() >= 25
            for H in (1, 5, 25):
                B = 211 if n_veh < 64 else 77           # not a multiple of any tile: a last block with idle env lanes
                obs0, tape, ri, pid, g_final, g5 = synthetic_case(m, task, B, H, seed=100 * n_veh + 10 * nf + H)
                got = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5)
                want = m.t_composed(obs0, tape, ri, pid, g_final, g5)
                what = '%s %s N%d nf%d H%d' % (task, mode, n_veh, nf, H)
                all_same(got, want, what)
                f5, fo = m.t_forward_tape(obs0, tape, ri, pid)
                assert same(got[0], f5) and same(got[1], fo), what + ': forward differs from eb_rollout_tape'
                assert bool(got[3].abs().sum() > 0) and bool(got[0][:, 1].abs().sum() > 0), what   # penalties and gradients are there
                n += 1
    assert n == 24


def test_large_batch_every_row_equals_the_composed_path():
    """65 536 x 32 x 25: every row's bits"""
    m = TapeModel('left', n_veh=32, n_future=0, mode='training')
    obs0, tape, ri, pid, g_final, g5 = synthetic_case(m, 'left', 65536, 25, seed=7)
    got = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5)
    want = m.t_composed(obs0, tape, ri, pid, g_final, g5)
    all_same(got, want, '65536 x 32 x 25')
    again = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5)
    all_same(again, got, '65536 x 32 x 25, second launch')


def test_forms_and_invariants():
    import torch
    m = TapeModel('right', n_veh=16, n_future=2, mode='training')
    B, H = 300, 25
    obs0, tape, ri, pid, g_final, g5 = synthetic_case(m, 'right', B, H, seed=3)
    full = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5)
    # two launches repeat their bits
    all_same(m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5), full, 'second launch')
    # the w5 form == a g_out5_steps array filled with the five values
    w5 = [-1.0, 10.0, 0.5, 0.25, 2.0]
    filled = torch.tensor(w5, device='cuda').view(1, 5, 1).expand(H, 5, B).contiguous()
    all_same(m.t_tape_vjp(obs0, tape, ri, pid, g_final, None, w5), m.t_tape_vjp(obs0, tape, ri, pid, g_final, filled), 'w5 form')
    # NULL cotangents are zero arrays
    z = m.t_tape_vjp(obs0, tape, ri, pid, None, None, None)
    assert not z[2].any() and not z[3].any() and same(z[0], full[0])
    a = m.t_tape_vjp(obs0, tape, ri, pid, None, None, w5)
    b = m.t_tape_vjp(obs0, tape, ri, pid, torch.zeros_like(g_final), filled)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    # value only == the forward of the full form; nothing else is written
    v = m.t_tape_vjp(obs0, tape, ri, pid, None, None, w5, g_obs0=False, g_tape=False)
    assert same(v[0], full[0]) and same(v[1], full[1]) and v[2] is None and v[3] is None
    only5 = m.t_tape_vjp(obs0, tape, ri, pid, None, None, w5, obs_out=False, g_obs0=False, g_tape=False)
    assert same(only5[0], full[0])
    # gradient of the tape alone (g_obs0 = NULL), of obs0 alone
    ga = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5, out5=False, obs_out=False, g_obs0=False)
    go = m.t_tape_vjp(obs0, tape, ri, pid, g_final, g5, out5=False, obs_out=False, g_tape=False)
    assert same(ga[3], full[3]) and same(go[2], full[2])
    # a batch permuted row-wise gives permuted bits; a slice gives the slice
    perm = torch.randperm(B, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    p = m.t_tape_vjp(obs0[perm].contiguous(), tape[:, perm].contiguous(), ri[perm].contiguous(), pid, g_final[perm].contiguous(),
                     g5[:, :, perm].contiguous())
    all_same(p, (full[0][:, :, perm], full[1][perm], full[2][perm], full[3][:, perm]), 'permuted batch')
    for first, n in ((0, 1), (77, 1), (5, 63), (100, 200)):
        s = slice(first, first + n)
        q = m.t_tape_vjp(obs0[s].contiguous(), tape[:, s].contiguous(), ri[s].contiguous(), pid, g_final[s].contiguous(),
                         g5[:, :, s].contiguous())
        all_same(q, (full[0][:, :, s], full[1][s], full[2][s], full[3][:, s]), 'slice %d+%d' % (first, n))
    # clipped actions get exact zeros (DAM:129)
    clipped = tape.abs() > 1.05
    assert bool(clipped.any()) and not full[3][clipped].any()


def test_refusals():
    m = TapeModel('left', n_veh=64, n_future=0, mode='training')
    limit = m.max_horizon()
    assert limit >= 25
    B = 8
    obs0, tape, ri, pid, g_final, g5 = synthetic_case(m, 'left', B, limit + 1, seed=1)
    with pytest.raises(ValueError) as e:                                   # horizon over the limit: EB_EINVAL, the limit in the message
        m.t_tape_vjp(obs0, tape, ri, pid, None, None, [1, 0, 0, 0, 0])
    assert str(limit) in str(e.value) and 'horizon' in str(e.value)
    ok = m.t_tape_vjp(obs0, tape[:limit].contiguous(), ri, pid, None, None, [1, 0, 0, 0, 0])     # at the limit it runs
    want = m.t_composed(obs0, tape[:limit].contiguous(), ri, pid, None,
                        m.torch.tensor([1.0, 0, 0, 0, 0], device='cuda').view(1, 5, 1).expand(limit, 5, B).contiguous())
    all_same(ok, want, 'horizon == limit')
    with pytest.raises(ValueError) as e:                                   # training mode without ref_idx
        m.t_tape_vjp(obs0, tape[:5].contiguous(), None, pid, None, None, [1, 0, 0, 0, 0])
    assert 'ref_idx' in str(e.value)
    # n_env == 0: a no-op that succeeds
    m.api.rollout_tape_vjp(m.h, 0, 5, None, None, None, 0, None, 0, None, None, None, None, None, None, m.stream)


@pytest.mark.parametrize('task,mode,nf', [('left', 'training', 0), ('straight', 'selecting', 2)])
def test_autograd_rollout_tape_equals_a_loop_of_rollout_step(task, mode, nf):
    import torch
    from env_build_amd import grad
    H, B = 25, 96
    dm = grad.DifferentiableEnvironmentModel(task, nf, mode=mode, n_veh=16)
    tm = TapeModel(task, n_veh=16, n_future=nf, mode=mode)
    obs0, tape, ri, pid, g_final, g5 = synthetic_case(tm, task, B, H, seed=11)
    nd = 9 + 3 * nf
    if mode == 'training':
        dm.reset(obs0, ri)
    else:
        dm.add_traj(obs0, 1)
    w5 = torch.tensor([-1.0, 10.0, 0.5, 0.25, 2.0], device='cuda')

    def loss_of(final, out5):
        return (final[:, :nd] * g_final).sum() + (out5 * w5.view(1, 5, 1)).sum()
    o1, t1 = obs0.clone().requires_grad_(True), tape.clone().requires_grad_(True)
    final, out5 = grad.rollout_tape(dm, o1, t1)
    g_o1, g_t1 = torch.autograd.grad(loss_of(final, out5), [o1, t1])
    o2, t2 = obs0.clone().requires_grad_(True), tape.clone().requires_grad_(True)
    obs, outs = o2, []
    for t in range(H):
        obs, o5 = grad.rollout_step(dm, obs, t2[t])
        outs.append(o5)
    g_o2, g_t2 = torch.autograd.grad(loss_of(obs, torch.stack(outs)), [o2, t2])
    assert same(final, obs.detach()) and same(out5, torch.stack(outs).detach())
    assert same(g_t1, g_t2) and same(g_o1[:, :nd], g_o2[:, :nd])
    assert not g_o1[:, nd:].any() and not torch.signbit(g_o1[:, nd:]).any()      # exact (+0) zeros in the vehicle columns
    assert bool(g_t1.abs().sum() > 0)
    # the method is left as it was: it raises
    with pytest.raises(_capi.EbError):
        dm.rollout_tape(tape)


def test_autograd_rollout_tape_beyond_the_limit_composes_step_launches():
    """a tape longer than eb_rollout_tape_vjp_max_horizon: grad.rollout_tape falls back to step launches + eb_rollout_chain_vjp,
    with the bits of the loop of grad.rollout_step"""
    import torch
    from env_build_amd import grad
    dm = grad.DifferentiableEnvironmentModel('right', 0, mode='training')
    tm = TapeModel('right', n_veh=NATIVE['right'], n_future=0, mode='training')
    H, B = grad.tape_vjp_max_horizon(dm) + 2, 24
    assert H - 2 == tm.max_horizon()
    obs0, tape, ri, pid, g_final, g5 = synthetic_case(tm, 'right', B, H, seed=5)
    dm.reset(obs0, ri)

    def loss_of(final, out5):
        return (final[:, :9] * g_final * 1e-3).sum() + (out5 * 1e-3).sum()
    o1, t1 = obs0.clone().requires_grad_(True), tape.clone().requires_grad_(True)
    final, out5 = grad.rollout_tape(dm, o1, t1)
    g1 = torch.autograd.grad(loss_of(final, out5), [o1, t1])
    o2, t2 = obs0.clone().requires_grad_(True), tape.clone().requires_grad_(True)
    obs, outs = o2, []
    for t in range(H):
        obs, o5 = grad.rollout_step(dm, obs, t2[t])
        outs.append(o5)
    g2 = torch.autograd.grad(loss_of(obs, torch.stack(outs)), [o2, t2])
    assert same(final, obs.detach()) and same(out5, torch.stack(outs).detach())
    assert same(g1[1], g2[1]) and same(g1[0][:, :9], g2[0][:, :9]) and not g1[0][:, 9:].any()
