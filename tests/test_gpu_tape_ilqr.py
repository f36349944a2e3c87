"""GPU (-m gpu): eb_rollout_tape_ilqr — one iLQR iteration on the model rollout in one launch (include/envbuild_ilqr.h,
csrc/eb_rollout_tape_ilqr.hip) — and mpc.ILQRMPC.

Exact: cand_out is ilqr.feedback_actions_reference fed the states a chain of eb_rollout_step launches produces for that tape; cost is
eb_rollout_tape_cand's cost over cand_out bit for bit (chunked by its limit); best_index is mpc.first_minimum(cost), best_cost / u_out /
x_out that candidate's bits; lq_out's A, B, l_z, l_u equal eb_rollout_step_vjp with unit cotangents numerically (+0 and -0 alike);
subsets of the outputs, permutation, repetition.
Bounded, by |v - v64| <= 4 E + 2^-20 max|v64| per column (tests/_grad_cases.py), E the restatement's own float32 run's distance from
its float64 run: l_zz / l_uu against ilqr.lq_reference, gains_out / dv against ilqr.riccati_reference on the kernel's own model; the
(row, step) pairs at which the two precisions or the kernel take different active sets are excluded together with every earlier step
of the row, at most 1 % of the pairs of each test, counted inside that test.  The kernel's set is read off its k: a component equal to the bound -1 - u or 1 - u is clamped."""
import numpy as np
import pytest

from tests._grad_cases import TASKS, MAX_EXCLUDED
from tests._tape import (ILQR_OUT as OUT, NATIVE, WEIGHTS, IlqrModel, bits, bound_check, diverged, edge_synthetic_case, load_example, mpc_setup,
                         same, same_numbers, synthetic_case)

pytestmark = pytest.mark.gpu
ALPHAS = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625)


def sets_from_k(k, u):
    """the active set per (step, env) read off k [H, 2, n] and the tape u [H, n, 2], in float32: index into ilqr.ACTIVE_SETS"""
    from env_build_amd.ilqr import ACTIVE_SETS
    f = np.float32
    k, u = np.asarray(k, f), np.moveaxis(np.asarray(u, f), 2, 1)
    state = np.where(k == f(-1) - u, 'L', np.where(k == f(1) - u, 'U', 'F'))
    names = np.char.add(state[:, 0], state[:, 1])
    return np.vectorize(ACTIVE_SETS.index)(names)


def new_count():
    return dict(pairs=0, excluded=0, alone=0)


def under_the_cap(count, what):
    """the (row, step) pairs a test's launches excluded, held to the cap of tests/_grad_cases.py inside the test that produced them"""
    print('%s: %d of %d (row, step) pairs excluded (the restatement alone: %d)' % (what, count['excluded'], count['pairs'], count['alone']))
    assert count['pairs'] > 0
    assert count['alone'] <= MAX_EXCLUDED * count['pairs'] and count['excluded'] <= MAX_EXCLUDED * count['pairs'], what


def check_launch(m, task, obs0, u_nom, ri, pid, what, count, x_nom=None, gains=None, alphas=(), mu=None, w5=WEIGHTS[0]):
    """one launch with every output, held to everything the header states -> its outputs; count (new_count) takes the pairs it excludes"""
    import torch
    from env_build_amd.mpc import first_minimum
    from env_build_amd.ilqr import feedback_actions_reference, lq_reference, riccati_reference, unpack_lq
    H, n = u_nom.shape[0], obs0.shape[0]
    K1 = 1 + len(alphas)
    out = m.t_ilqr(obs0, u_nom, ri, pid, x_nom, gains, alphas, mu, w5)
    for k in OUT:
        assert not bool(torch.isnan(out[k].float()).any()) and (k != 'best_index' or int(out[k].min()) >= 0), '%s: %s has unwritten entries' % (what, k)
    cand = out['cand']
    # the tapes: the restatement fed the states the step kernel's chain produces for that very tape
    pre = m.chain_states(obs0, cand, ri, pid)                                   # [K1, H, n, D]
    for j in range(K1):
        x = pre[j, :, :, :6].permute(0, 2, 1).cpu().numpy()
        want = feedback_actions_reference(u_nom.cpu().numpy(), x, None if x_nom is None else x_nom.cpu().numpy(),
                                          None if gains is None else gains.cpu().numpy(), None if j == 0 else alphas[j - 1])
        assert np.array_equal(cand[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), '%s: candidate %d differs from the restatement in %d words' % (
            what, j, int((cand[j].cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum()))
    cost = m.cand_cost(obs0, cand, ri, pid, w5)
    assert same(out['cost'], cost), '%s: cost differs from eb_rollout_tape_cand in %d of %d words' % (
        what, int((bits(out['cost']) != bits(cost)).sum()), cost.numel())
    idx = first_minimum(cost)
    assert torch.equal(out['best_index'].long(), idx), what
    assert same(out['best_cost'], cost.gather(0, idx.view(1, n))[0]), what
    assert same(out['u'], cand.gather(0, idx.view(1, 1, n, 1).expand(1, H, n, 2))[0]), what
    best_pre = pre.gather(0, idx.view(1, 1, n, 1).expand(1, H, n, m.D))[0]      # [H, n, D]
    assert same(out['x'], best_pre[:, :, :6].permute(0, 2, 1).contiguous()), what
    # the model's first-order part against the step VJP
    M = unpack_lq(out['lq'].cpu().numpy())
    rows = m.unit_vjps(best_pre, out['u'], ri, pid, w5).cpu()
    t = torch.from_numpy
    assert same_numbers(t(M['A']), rows[:, :, :9, :9]) and same_numbers(t(M['B']), rows[:, :, :9, 9:]), '%s: A / B' % what
    assert same_numbers(t(np.ascontiguousarray(M['l_z'])), rows[:, :, 9, :9]), '%s: l_z' % what
    assert same_numbers(t(np.ascontiguousarray(M['l_u'])), rows[:, :, 9, 9:]), '%s: l_u' % what
    # the second-order part and the sweep against the float64 restatement
    nd = m.D - 4 * m.n_veh
    flat, act = best_pre.reshape(H * n, m.D).cpu().numpy(), out['u'].reshape(H * n, 2).cpu().numpy()
    z32, u32 = lq_reference(task, flat, act, w5, nd, np.float32)
    z64, u64 = lq_reference(task, flat, act, w5, nd, np.float64)
    iu = np.triu_indices(9)
    finite = np.isfinite(flat).all(1)
    bound_check(M['l_zz'].reshape(H * n, 9, 9)[:, iu[0], iu[1]], z32[:, iu[0], iu[1]], z64[:, iu[0], iu[1]], finite, what + ' l_zz')
    bound_check(M['l_uu'].reshape(H * n, 2), u32, u64, finite, what + ' l_uu')
    mu_np = None if mu is None else mu.cpu().numpy()
    u_np = out['u'].cpu().numpy()
    args = (M['A'], M['B'], M['l_z'], M['l_u'], M['l_zz'], M['l_uu'], u_np, mu_np)
    g32, dv32, s32 = riccati_reference(*args, dtype=np.float32)
    g64, dv64, s64 = riccati_reference(*args, dtype=np.float64)
    gains_out, dv = out['gains'].cpu().numpy(), out['dv'].cpu().numpy()
    zero_k = np.zeros((H, 2, n), np.float32)
    as_k = lambda s, g: np.where(s[:, None, :] < 0, zero_k, g[:, 0:2].astype(np.float32))   # the fallback's k is zero
    ref_sets = sets_from_k(as_k(s64, g64), u_np)
    bad_alone = diverged(sets_from_k(as_k(s32, g32), u_np), ref_sets)
    bad = bad_alone | diverged(sets_from_k(gains_out[:, 0:2], u_np), ref_sets) | ~finite.reshape(H, n)
    count['pairs'] += H * n; count['excluded'] += int(bad.sum()); count['alone'] += int(bad_alone.sum())
    bound_check(np.moveaxis(gains_out, 1, 2), np.moveaxis(g32, 1, 2), np.moveaxis(g64, 1, 2), ~bad, what + ' gains')
    bound_check(dv.T, dv32.T, dv64.T, (~bad).all(0), what + ' dv')
    return out


def random_gains(n, H, seed):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    gains = torch.randn((H, 14, n), device='cuda', generator=g) * 0.05
    gains[:, 0:2] *= 6.0
    x_nom = torch.randn((H, 6, n), device='cuda', generator=g)
    return x_nom, gains


def two_launches(m, task, obs0, tape, ri, pid, n_alpha, what, count, w5=WEIGHTS[0], mu=None, seed=0):
    """launch 0 without gains, then a launch with gains from launch 0, then one with gains drawn at random around launch 0's states"""
    first = check_launch(m, task, obs0, tape, ri, pid, what + ' launch 0', count, w5=w5)
    if n_alpha == 0:
        return first
    al = ALPHAS[:n_alpha]
    second = check_launch(m, task, obs0, first['u'], ri, pid, what + ' launch 1', count, first['x'], first['gains'], al, mu, w5)
    xr, gr = random_gains(obs0.shape[0], tape.shape[0], seed)
    check_launch(m, task, obs0, tape, ri, pid, what + ' random gains', count, (first['x'] + 0.05 * xr).contiguous(), gr.contiguous(), al, mu, w5)
    return second


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_shape_grid(task, mode):
    """n_env in {1, 3, 9}, H in {1, 2, 25}, n_veh in {native, 16, 64}, n_future in {0, 2}, n_alpha in {0, 1, 7 = max} — NOT their full
    product: a rotation over the six (task, mode) pairs, four cases each; over the pairs every value of every factor meets every
    task.  The weights (zeros in different rows) and mu rotate with them."""
    import torch
    base = TASKS.index(task) * 2 + (mode == 'selecting')
    count = new_count()
    for i in range(4):
        k = base + i
        n_veh, nf = (NATIVE[task], 16, 64)[k % 3], (0, 2)[(k // 3) % 2]
        H, B, n_alpha = (25, 1, 2)[(k + i) % 3], (1, 3, 9)[(k // 2 + i) % 3], (7, 0, 1, 7)[(k + i // 2) % 4]
        m = IlqrModel(task, n_veh=n_veh, n_future=nf, mode=mode)
        assert m.ilqr_max(25) == (7, m.ilqr_max(1)[1]) and m.ilqr_max()[1] >= 25
        obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, task, B, H, seed=10 * k + i)
        mu = torch.linspace(0.0, 1.0, B, device='cuda') if k % 2 else None
        two_launches(m, task, obs0, tape, ri, pid, n_alpha, '%s %s B%d H%d N%d nf%d a%d' % (task, mode, B, H, n_veh, nf, n_alpha),
                     count, w5=WEIGHTS[(0, 3, 2, 0)[k % 4]], mu=mu, seed=k)
    under_the_cap(count, 'grid %s %s' % (task, mode))


@pytest.mark.parametrize('task', TASKS)
def test_crowded_remote_and_near_wall_scenes(task):
    """every vehicle within 4.5 m of its ego, a third of the egos off the closest-point cell grid, a third on the lane's walls, ids out
    of range (edge_synthetic_case), at 32 and 64 slots: eight and four envs per block, idle env slots in the last block.  Both cases
    hold more than 200 (row, step) pairs: the factor 4 of the bound covers a sample maximum over a few hundred of them
    (tests/_grad_cases.py), and E taken over a few dozen is not that maximum."""
    count = new_count()
    for n_veh, mode, B, H in ((32, 'training', 9, 25), (64, 'selecting', 10, 25)):
        m = IlqrModel(task, n_veh=n_veh, n_future=0, mode=mode)
        obs0, tape, ri, pid, _g, _g5 = edge_synthetic_case(m, task, 120, H, seed=n_veh)      # (the helper wants its far egos)
        obs0, tape, ri = obs0[:B].contiguous(), tape[:, :B].contiguous(), None if ri is None else ri[:B].contiguous()
        out = two_launches(m, task, obs0, tape, ri, pid, 7, 'edge %s N%d' % (task, n_veh), count, w5=WEIGHTS[3], seed=n_veh)
        assert bool((out['cost'] > 0).all())
    under_the_cap(count, 'edge %s' % task)


def test_independence():
    """any subset of the outputs has the full set's bits; a permuted batch gives permuted bits; two launches repeat"""
    import torch
    m = IlqrModel('right', n_veh=16, n_future=2, mode='training')
    B, H = 9, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'right', B, H, seed=3)
    first = m.t_ilqr(obs0, tape, ri, pid)
    mu = torch.linspace(0.0, 0.5, B, device='cuda')
    kw = dict(x_nom=first['x'], gains=first['gains'], alphas=ALPHAS, w5=WEIGHTS[3])
    full = m.t_ilqr(obs0, first['u'], ri, pid, mu=mu, **kw)
    again = m.t_ilqr(obs0, first['u'], ri, pid, mu=mu, **kw)
    for k in OUT:
        assert same(full[k], again[k]), k
    assert int(full['best_index'].max()) > 0, 'some env accepts a step'
    for want in (('cost',), ('best_index', 'best_cost'), ('u',), ('x',), ('gains',), ('dv',), ('cand',), ('lq',), ('u', 'x', 'cost'),
                 ('gains', 'dv', 'u', 'x', 'best_index')):
        part = m.t_ilqr(obs0, first['u'], ri, pid, mu=mu, want=want, **kw)
        for k in want:
            assert same(part[k], full[k]), 'subset %r: %s' % (want, k)
    perm = torch.randperm(B, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    p = m.t_ilqr(obs0[perm].contiguous(), first['u'][:, perm].contiguous(), ri[perm].contiguous(), pid, mu=mu[perm].contiguous(),
                 x_nom=first['x'][:, :, perm].contiguous(), gains=first['gains'][:, :, perm].contiguous(), alphas=ALPHAS, w5=WEIGHTS[3])
    for k in ('cost', 'best_index', 'best_cost', 'x', 'gains', 'dv', 'lq'):
        assert same(p[k], full[k][..., perm].contiguous()), 'permuted %s' % k
    for k in ('u', 'cand'):
        assert same(p[k], full[k][..., perm, :].contiguous()), 'permuted %s' % k
    s = slice(4, 5)
    q = m.t_ilqr(obs0[s].contiguous(), first['u'][:, s].contiguous(), ri[s].contiguous(), pid, mu=mu[s].contiguous(),
                 x_nom=first['x'][:, :, s].contiguous(), gains=first['gains'][:, :, s].contiguous(), alphas=ALPHAS, w5=WEIGHTS[3])
    for k in ('cost', 'best_index', 'best_cost', 'x', 'gains', 'dv', 'lq'):
        assert same(q[k], full[k][..., s].contiguous()), 'slice %s' % k


def test_a_nan_row_leaves_the_others_alone_and_candidate_0_is_the_tape_vjp_value():
    """a NaN row of obs0: NaN costs, index 0, the other envs' bits unchanged.  Without gains candidate 0's cost agrees with
    eb_rollout_tape_vjp's value path (cost_from_out5 of its out5: another summation order of the same terms)"""
    import torch
    from env_build_amd.mpc import cost_from_out5
    m = IlqrModel('straight', n_veh=16, n_future=0, mode='training')
    B, H = 3, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'straight', B, H, seed=4)
    first = m.t_ilqr(obs0, tape, ri, pid)
    o5, _oo, _g0, _gt = m.t_tape_vjp(obs0, first['u'], ri, pid, w5=WEIGHTS[0], obs_out=False, g_obs0=False, g_tape=False)
    J = cost_from_out5(o5, WEIGHTS[0])
    assert float((first['cost'][0] - J).abs().max()) <= 1e-5 * float(J.abs().max()) + 1e-5
    per_step = sum(o5[:, k] * WEIGHTS[0][k] for k in range(5) if WEIGHTS[0][k] != 0.0)
    Jseq = torch.zeros(B, device='cuda')
    for t in range(H):
        Jseq = Jseq + per_step[t]
    assert same(first['cost'][0], Jseq), 'candidate 0: the ascending-t sum of the value path\'s steps, bit for bit'
    kw = dict(x_nom=first['x'], gains=first['gains'], alphas=ALPHAS[:3])
    clean = m.t_ilqr(obs0, first['u'], ri, pid, **kw)
    rows = obs0.clone()
    rows[1, 3] = float('nan')
    b = m.t_ilqr(rows, first['u'], ri, pid, **kw)
    keep = [0, 2]
    for k in ('cost', 'best_index', 'best_cost', 'x', 'gains', 'dv', 'lq'):
        assert same(b[k][..., keep], clean[k][..., keep]), k
    for k in ('u', 'cand'):
        assert same(b[k][..., keep, :], clean[k][..., keep, :]), k
    assert bool(torch.isnan(b['cost'][:, 1]).all()) and int(b['best_index'][1]) == 0 and bool(torch.isnan(b['best_cost'][1]))
    assert same(b['u'][:, 1], b['cand'][0, :, 1])
    # a step whose Q is not finite gets k = K = 0, so no NaN ever reaches the gains (the last steps' Q_uu / Q_u do not depend on x: finite)
    assert bool(torch.isfinite(b['gains'][:, :, 1]).all()) and not bool(b['gains'][0, :, 1].any())


def test_refusals():
    import torch
    from env_build_amd import _capi
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.ilqr import rollout_tape_ilqr, tape_ilqr_max
    m = IlqrModel('left', n_veh=64, n_future=0, mode='training')
    max_alpha, max_h = m.ilqr_max()
    assert max_alpha >= 7 and max_h >= 25
    B, H = 4, 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=1)
    first = m.t_ilqr(obs0, tape, ri, pid)
    ok = dict(ri=ri, path_id=pid, x_nom=first['x'], gains=first['gains'], alphas=ALPHAS[:2])
    m.t_ilqr(obs0, first['u'], **ok)
    bad = [dict(x_nom=None), dict(gains=None),                                 # one of x_nom / gains without the other
           dict(x_nom=None, gains=None),                                       # n_alpha > 0 without gains
           dict(alphas=(1.0, 0.0)), dict(alphas=(1.0, -0.5)), dict(alphas=(float('nan'), 1.0)), dict(alphas=(float('inf'),)),
           dict(alphas=(0.5,) * (max_alpha + 1)),                              # over the limit
           dict(w5=None), dict(w5=(1.0, 10.0, 0, 0, 0)), dict(w5=(-1.0, -10.0, 0, 0, 0)), dict(w5=(-1.0, 1.0, 0, 0, float('nan'))),
           dict(ri=None)]                                                      # training mode without ref_idx
    for kw in bad:
        with pytest.raises(ValueError):
            m.t_ilqr(obs0, first['u'], **dict(ok, **kw))
    with pytest.raises(ValueError) as e:                                       # horizon beyond the limit: the limit in the message
        m.t_ilqr(obs0, torch.zeros((max_h + 1, B, 2), device='cuda'), ri, pid)
    assert str(max_h) in str(e.value)
    with pytest.raises(ValueError):                                            # an output pointer equal to an input pointer
        m.t_ilqr(obs0, first['u'], out=dict(u=first['u']), want=('u',), **ok)
    with pytest.raises(ValueError):
        m.t_ilqr(obs0, first['u'], out=dict(gains=first['gains']), want=('gains',), **ok)
    sel = IlqrModel('left', n_veh=8, n_future=0, mode='selecting')
    o8, t8, _ri, _pid, _g, _g5 = synthetic_case(sel, 'left', B, H, seed=2)
    for p in (3, -1):
        with pytest.raises(ValueError):                                        # a path id out of range in selecting mode
            sel.t_ilqr(o8, t8, None, p)
    # n_env == 0: a no-op that succeeds
    m.api.rollout_tape_ilqr(m.h, 0, 5, 0, *([None] * 5), 0, *([None] * 12), m.stream)
    # the facade: one launch, the raw entry's bits
    model = EnvironmentModel('left', 0, mode='training', n_veh=64)
    assert tape_ilqr_max(model, H) == (max_alpha, max_h)
    a = rollout_tape_ilqr(model, obs0, tape, ref_indexes=ri, want=('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv', 'cand', 'lq'))
    for k in OUT:
        assert same(a[k], first[k]), k
    mu = torch.full((B,), 0.25, device='cuda')
    b = rollout_tape_ilqr(model, obs0, a['u'], a['x'], a['gains'], alphas=ALPHAS[:2], mu=mu, ref_indexes=ri)
    raw = m.t_ilqr(obs0, first['u'], mu=mu, **ok)
    for k in ('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv'):
        assert same(b[k], raw[k]), k
    with pytest.raises(_capi.EbError):                                         # fp16 state has no iLQR form
        rollout_tape_ilqr(EnvironmentModel('left', 0, mode='training', state_dtype='float16'), obs0, tape)
    with pytest.raises(ValueError):
        rollout_tape_ilqr(model, obs0, tape, want=('nothing',), ref_indexes=ri)


# ---- the solver ----
@pytest.mark.parametrize('task', TASKS)
def test_ilqr_mpc_on_the_g17_start_states(task):
    """J_history never increases; J <= J of the start (both by the same independent evaluation); u in the box; launches ==
    iterations + 2; a second solve repeats its bits.  The rows that agree with the reference optimiser under the J <= J_ref + 0.1 rule
    and the launches it takes to reach the default solver's final J are printed, not asserted (DESIGN.md §14 records them)."""
    import torch
    from env_build_amd.mpc import ILQRMPC
    z, model, mpc, obs0, ref = mpc_setup(task)
    H, B = int(z['horizon']), obs0.shape[0]
    impc = ILQRMPC(model, horizon=H)
    u, J, info = impc.solve(obs0, ref_indexes=ref)
    hist = info['J_history']
    assert u.shape == (H, B, 2) and float(u.abs().max()) <= 1.0 and bool(torch.isfinite(J).all())
    assert hist.shape == (impc.iterations + 1, B) and bool((hist[1:] <= hist[:-1]).all()) and same(hist[-1], info['J_kernel'])
    assert info['launches'] == impc.iterations + 2 and info['best_index'].shape == (impc.iterations, B) and info['mu'].shape == (B,)
    J_init = mpc.value_and_grad(obs0, torch.zeros_like(u), ref, 0, need_grad=False)[0]
    assert bool((J <= J_init).all()) and bool((J < J_init).any())
    assert same(J, mpc.value_and_grad(obs0, u, ref, 0, need_grad=False)[0])
    assert float((J - info['J_kernel']).abs().max()) <= 1e-5 * float(J.abs().max()) + 1e-5    # two summation orders of one cost
    u2, J2, info2 = impc.solve(obs0, ref_indexes=ref)
    assert same(u2, u) and same(J2, J) and same(info2['J_history'], hist) and same(info2['mu'], info['mu'])
    _ud, J_default, _ = mpc.solve(obs0, ref_indexes=ref)
    reached = (hist <= J_default.view(1, B) + 1e-5 * J_default.abs().view(1, B))
    first = torch.where(reached.any(0), reached.int().argmax(0) + 2, torch.full((B,), -1, device=hist.device))
    agree = J.double().cpu().numpy() <= z['J_ref'] + 0.1
    print('g17 %s ILQRMPC alone (%d iterations): %d of %d rows disagree with J_ref + 0.1; mean J %.3f (default solver %.3f, J_ref %.3f); '
          'launches to reach the default solver\'s final J per row (-1: not reached): %s'
          % (task, impc.iterations, int((~agree).sum()), B, float(J.mean()), float(J_default.mean()), float(z['J_ref'].mean()),
             first.tolist()))


@pytest.mark.parametrize('task', TASKS)
def test_polished_ilqr_never_ends_above_the_default_solver(task):
    """polish: the zero tape and the iLQR tape both descend; start 0's descent is the default solver's, so J <= J_default on EVERY row"""
    import torch
    from env_build_amd.mpc import ILQRMPC, OpenLoopMPC
    z, model, mpc, obs0, ref = mpc_setup(task)
    H, B = int(z['horizon']), obs0.shape[0]
    _ud, J_default, _info_d = mpc.solve(obs0, ref_indexes=ref)
    hybrid = ILQRMPC(model, horizon=H, polish=OpenLoopMPC(model, horizon=H))
    u, J, info = hybrid.solve(obs0, ref_indexes=ref)
    assert float(u.abs().max()) <= 1.0 and bool(torch.isfinite(J).all())
    assert same(info['polish']['J_starts'][0], J_default), 'start 0 of the polish is not the default solver bit for bit'
    assert bool((J <= J_default).all())
    assert info['launches'] == hybrid.iterations + 2 + info['polish']['launches']
    disagree = int((J.double().cpu().numpy() > z['J_ref'] + 0.1).sum())
    default = int((J_default.double().cpu().numpy() > z['J_ref'] + 0.1).sum())
    print('g17 %s ILQRMPC + polish: %d of %d rows disagree (default solver: %d); %d rows end below the default solver'
          % (task, disagree, B, default, int((J < J_default).sum())))
    assert disagree <= default
    with pytest.raises(ValueError):
        ILQRMPC(model, horizon=H, polish=OpenLoopMPC(model, horizon=H - 1))
    with pytest.raises(ValueError):
        ILQRMPC(model, horizon=H, weights=(1.0, 10.0, 0.0, 0.0, 0.0))


def test_ilqr_example_runs_a_few_control_steps():
    import torch
    mod = load_example('mpc_ilqr')
    r = mod.run(n_env=128, control_steps=3, iterations=4)
    assert torch.isfinite(r['J_first']).all() and torch.isfinite(r['reward_sum']).all() and torch.isfinite(r['J_last']).all()
    slack = 1e-5 * r['J0_first'].abs() + 1e-5              # J0 is the kernel's sum, J the independent evaluation's
    assert bool((r['J_first'] <= r['J0_first'] + slack).all()) and bool((r['J_first'] < r['J0_first']).any())
    assert r['launches'] == 3 * (4 + 2)
