"""GPU (-m gpu): eb_rollout_tape_cand_vjp — cost AND gradient of K candidate action tapes per env from one shared scene in one launch
(include/envbuild_cand_grad.h, csrc/eb_rollout_tape_cand_vjp.hip).

Bit for bit, for every candidate k: out5_steps[k] == eb_rollout_tape, cost[k] == eb_rollout_tape_cand, g_action_tapes[k] and
g_obs0[k] == eb_rollout_tape_vjp on (obs0, tapes[k], candidate k's path, the same w5); per-candidate paths with retrack against rows
rebuilt through ReferencePath.tracking_error_vector_batched; independence; refusals; chunks.  Against the reference directly: the
G19 fixtures (scripts/gen_golden_mpc_paths.py), the three paths as the three candidates of ONE launch, under the column rule of
tests/_grad_cases.py.  The consumers: cand.rollout_tape_candidates_grad, OpenLoopMPC.solve(starts='all') on the G17 rows,
OpenLoopMPC.solve_paths on the G19 rows, examples/mpc_paths.py.

Agreement with the reference's optimiser follows tests/test_gpu_mpc.py: a row agrees when J <= J_ref + 0.1 (G19: Jbest_ref = the
minimum over the paths), 0.1 being the reference's own stopping tolerance; at most one quarter of a file's rows may disagree.

Measured on an MI355X (60 iterations, the defaults), rows that disagree: solve(starts='all') with the starts zero, (0, -1), (0, +1) on
G17: left 2 of 9, straight 1 of 16, right 2 of 16 (the single-start solver in the same run: 2, 2, 3); solve_paths on G19: left 2 of 9,
straight 1 of 16, right 4 of 16 (the float64 run of the same lines on the reference's cost: 2, 2, 4; the reference alone: 2, 0, 0),
and 9 of 9, 15 of 16, 15 of 16 rows pick the reference's best path.  Start k of a K-start solve repeats the bits of the single-start
solve from U[k] on the GPU as it does on the CPU (asserted below)."""
import ctypes as C

import numpy as np
import pytest

from env_build_amd import _capi
from tests._helpers import golden
from tests._grad_cases import TASKS, check_columns, column_tolerance, edge_cases
from tests._tape import (NATIVE, WEIGHTS, CandGradModel, bits, candidate_tapes, edge_synthetic_case, load_example, mpc_setup, retracked_rows,
                         same, synthetic_case)

pytestmark = pytest.mark.gpu


def check_against_the_parents(m, obs0, tapes, ri, pid, what, w5):
    """one eb_rollout_tape_cand_vjp launch against eb_rollout_tape / eb_rollout_tape_cand / eb_rollout_tape_vjp, candidate by candidate"""
    o5, J, g0, gt = m.t_cand_vjp(obs0, tapes, ri, 0, None, pid, False, w5)
    _o5c, Jc = m.t_cand(obs0, tapes, ri, 0, None, pid, False, w5, out5=False)
    assert same(J, Jc), '%s: cost differs from eb_rollout_tape_cand in %d of %d words' % (what, int((bits(J) != bits(Jc)).sum()), J.numel())
    for k in range(tapes.shape[0]):
        f5, _ = m.t_forward_tape(obs0, tapes[k], ri, pid)
        _v5, _oo, v0, vt = m.t_tape_vjp(obs0, tapes[k], ri, pid, w5=w5, out5=False, obs_out=False)
        for name, a, b in (('out5_steps', o5[k], f5), ('g_action_tapes', gt[k], vt), ('g_obs0', g0[k], v0)):
            assert same(a, b), '%s: candidate %d: %s differs in %d of %d words' % (what, k, name, int((bits(a) != bits(b)).sum()), b.numel())
    return o5, J, g0, gt


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_every_candidate_has_the_bits_of_the_parent_entries(task, mode):
    """n_veh in {native, 16, 32, 64} x H in {1, 5, 25} x n_future in {0, 2} x K in {1, 2, 3, the reported limit}; batches that leave
    idle lanes in the last block; actions beyond +-1.05; out-of-range ref_idx (synthetic_case); weights with zeros in different rows
    and all zero"""
    n = 0
    for n_veh in (NATIVE[task], 16, 32, 64):
        for nf in (0, 2):
            m = CandGradModel(task, n_veh=n_veh, n_future=nf, mode=mode)
            assert m.cand_grad_max(25) == min(8, 65536 // (176 * n_veh + 384 * 25)) >= (4 if n_veh <= 32 else 3)
            for H in (1, 5, 25):
                limit = m.cand_grad_max(H)
                assert limit == min(8, 65536 // (176 * n_veh + 384 * H)) and limit <= m.cand_max(H)
                B = 211 if n_veh < 64 else 77           # not a multiple of any tile: a last block with idle env lanes
                obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, task, B, H, seed=100 * n_veh + 10 * nf + H)
                for K in sorted({1, 2, 3, limit}):
                    tapes = candidate_tapes(m, tape, K, seed=K)
                    assert K == 1 or bool((tapes.abs() > 1.05).any())
                    w5 = WEIGHTS[n % len(WEIGHTS)]
                    o5, J, g0, gt = check_against_the_parents(m, obs0, tapes, ri, pid, '%s %s N%d nf%d H%d K%d' % (task, mode, n_veh, nf, H, K), w5)
                    assert bool(m.torch.isfinite(gt).all()) and bool(m.torch.isfinite(g0).all())
                    assert bool(g0[:, :, 9:].abs().sum() == 0)
                    if not any(w5):                     # all weights zero: every cotangent is zero
                        assert not bool(gt.any()) and not bool(g0.any())
                    if w5[0] != 0.0:                    # the reward row holds -5 steer^2 - 0.05 a_x^2 (DAM:198-199, 297-298)
                        assert bool(gt.abs().sum() > 0)
                    n += 1
    assert n >= 24 * 3


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_crowded_remote_and_near_wall_scenes_in_every_tile_shape(task, mode):
    """32 and 64 slots, every vehicle within 4.5 m of its ego (every (record, candidate) pair in the near queue), a third of the egos
    off the closest-point cell grid, a third on the lane's walls (edge_synthetic_case), with batch sizes and horizons that let the
    launch pick each tile shape its LDS layout allows (32, 16 or 8 envs per block), each batch leaving idle lanes in its last block"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 0
    for n_veh in (32, 64):
        m = CandGradModel(task, n_veh=n_veh, n_future=0, mode=mode)
        for E, K, H in ((32, 2, 5), (16, 2, 5), (16, 3, 5), (16, 4, 5), (8, 3, 25), (8, m.cand_grad_max(25), 25)):
            if E * n_veh > 1024 or E * K * (22 * n_veh + 48 * H) > 65536:
                continue
            B = 2 * n_cu * E + 11 if E > 8 else 211
            obs0, tape, ri, pid, _g, _g5 = edge_synthetic_case(m, task, B, H, seed=1000 * n_veh + E + K)
            tapes = candidate_tapes(m, tape, K, seed=E)
            o5, _J, _g0, gt = check_against_the_parents(m, obs0, tapes, ri, pid, '%s %s N%d E%d K%d B%d' % (task, mode, n_veh, E, K, B), WEIGHTS[n % 4])
            assert bool((o5[0, 0, 3] > 0).all()) and bool(torch.isfinite(gt).all())
            n += 1
    assert n >= 7


@pytest.mark.parametrize('task', TASKS)
def test_the_edge_chains_as_candidates(task):
    """the G18 chains (starts on the junction's exit side and next to the entry lane's walls) as candidate 1 of 3"""
    for c in edge_cases(task)[1]:
        m = CandGradModel(task, n_veh=c.n_veh, n_future=c.n_future, mode=c.mode)
        ri = None if c.ref_idx() is None else m.to_dev(c.ref_idx(), np.int32)
        tape = m.to_dev(c['tape'])
        K = min(3, m.cand_grad_max(tape.shape[0]))
        tapes = candidate_tapes(m, tape, 3, seed=18)[[1, 0, 2][:K]].contiguous()
        check_against_the_parents(m, m.to_dev(c['obs0']), tapes, ri, c.path_id, 'g18 %s %s' % (task, c.name), WEIGHTS[3])


def test_large_batch_every_row_and_candidate():
    """65 536 x 32 x 25 x 3: every row's and candidate's bits; a second launch repeats them"""
    m = CandGradModel('left', n_veh=32, n_future=0, mode='training')
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', 65536, 25, seed=7)
    tapes = candidate_tapes(m, tape, 3, seed=7)
    first = check_against_the_parents(m, obs0, tapes, ri, pid, '65536 x 32 x 25 x 3', WEIGHTS[0])
    again = m.t_cand_vjp(obs0, tapes, ri, 0, None, pid, False, WEIGHTS[0])
    assert all(same(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_per_candidate_paths_with_retrack(task, mode):
    """[K, B] ref_idx (training, with out-of-range ids) and path_ids (selecting) with retrack=True, against eb_rollout_tape_vjp on rows
    whose tracking columns were replaced for that candidate's path.  obs0's own tracking columns are NaN: retrack reads none of them."""
    import torch
    from env_build_amd.cand import rollout_tape_candidates, rollout_tape_candidates_grad
    from env_build_amd.dynamics_and_models import EnvironmentModel
    for n_veh, nf in ((None, 0), (16, 2), (64, 0)):
        model = EnvironmentModel(task, nf, mode=mode, n_veh=n_veh)
        tm = CandGradModel(task, n_veh=model.veh_num, n_future=nf, mode=mode)
        B, H, K = 203, 25, 3
        obs0, tape, _ri, _pid, _g, _g5 = synthetic_case(tm, task, B, H, seed=31 + nf)
        tapes = candidate_tapes(tm, tape, K, seed=5)
        shared = obs0.clone()
        shared[:, 6:9 + 3 * nf] = float('nan')
        w5 = WEIGHTS[3]
        if mode == 'training':
            g = torch.Generator(device='cuda').manual_seed(2)
            ri = torch.randint(0, 3, (K, B), device='cuda', generator=g, dtype=torch.int32)
            ri[1, ::9], ri[2, ::13] = 5, -1                # out of range: zero tracking (DAM:342, 352)
            kw = dict(ref_indexes=ri)
        else:
            ids = [2, 0, 1]
            kw = dict(path_indexes=ids)
        cost, g_tapes, out5, g_obs = rollout_tape_candidates_grad(model, shared, tapes, w5, retrack=True, want_out5=True, want_g_obs=True, **kw)
        v5, vcost = rollout_tape_candidates(model, shared, tapes, retrack=True, weights=w5, **kw)
        assert same(out5, v5) and same(cost, vcost) and bool(torch.isfinite(g_tapes).all()) and bool(torch.isfinite(g_obs).all())
        for k in range(K):
            if mode == 'training':
                rk = ri[k].contiguous()
                rows = retracked_rows(model, obs0, nf, rk)
                _o5, _oo, v0, vt = tm.t_tape_vjp(rows, tapes[k], rk, 0, w5=w5, out5=False, obs_out=False)
            else:
                model.ref_path.set_path(ids[k])
                rows = retracked_rows(model, obs0, nf)
                _o5, _oo, v0, vt = tm.t_tape_vjp(rows, tapes[k], None, ids[k], w5=w5, out5=False, obs_out=False)
            what = '%s %s N%d nf%d: candidate %d' % (task, mode, model.veh_num, nf, k)
            assert same(g_tapes[k], vt), what + ' g_action_tapes'
            assert same(g_obs[k], v0), what + ' g_obs0'


def test_independence():
    """a permuted batch gives permuted bits, a slice the slice; permuting the candidates permutes the outputs; two launches repeat
    their bits; a candidate's bits do not depend on its neighbours in the set (NaN tapes next to it)"""
    import torch
    m = CandGradModel('right', n_veh=16, n_future=2, mode='training')
    B, H, K = 300, 25, 4
    assert m.cand_grad_max(H) >= K
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'right', B, H, seed=3)
    tapes = candidate_tapes(m, tape, K, seed=3)
    w5 = WEIGHTS[3]
    run = lambda o, t, r: m.t_cand_vjp(o, t, r, 0, None, pid, False, w5)
    full = run(obs0, tapes, ri)
    assert all(same(a, b) for a, b in zip(full, run(obs0, tapes, ri)))
    perm = torch.randperm(B, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    p = run(obs0[perm].contiguous(), tapes[:, :, perm].contiguous(), ri[perm].contiguous())
    assert same(p[0], full[0][:, :, :, perm]) and same(p[1], full[1][:, perm]) and same(p[2], full[2][:, perm]) and same(p[3], full[3][:, :, perm])
    for first, n in ((0, 1), (77, 1), (5, 63), (100, 200)):
        s = slice(first, first + n)
        q = run(obs0[s].contiguous(), tapes[:, :, s].contiguous(), ri[s].contiguous())
        assert same(q[0], full[0][:, :, :, s]) and same(q[1], full[1][:, s]) and same(q[2], full[2][:, s]) and same(q[3], full[3][:, :, s]), 'slice %d+%d' % (first, n)
    order = [2, 0, 3, 1]
    c = run(obs0, tapes[order].contiguous(), ri)
    assert all(same(a, b[order]) for a, b in zip(c, full))
    for k in range(K):                                    # alone among NaN tapes, and alone in a set of one
        lonely = torch.full_like(tapes, float('nan'))
        lonely[k] = tapes[k]
        a = run(obs0, lonely, ri)
        one = run(obs0, tapes[k:k + 1].contiguous(), ri)
        assert all(same(x[k], f[k]) for x, f in zip(a, full)) and all(same(x[0], f[k]) for x, f in zip(one, full))
    # the optional outputs left out: the same gradient bits
    bare = m.t_cand_vjp(obs0, tapes, ri, 0, None, pid, False, w5, out5=False, cost=False, g_obs0=False)
    assert bare[0] is None and bare[1] is None and bare[2] is None and same(bare[3], full[3])
    shared = m.t_cand_vjp(obs0, tapes, ri.view(1, B).expand(K, B).contiguous(), B, None, pid, False, w5)
    assert all(same(a, b) for a, b in zip(shared, full))


def test_refusals_and_chunks():
    import torch
    from env_build_amd.cand import rollout_tape_candidates_grad, tape_cand_grad_max
    from env_build_amd.dynamics_and_models import EnvironmentModel
    m = CandGradModel('left', n_veh=64, n_future=0, mode='training')
    B, H = 40, 25
    limit = m.cand_grad_max(H)
    assert limit == 3 and m.cand_grad_max(128) == 1 and m.cand_grad_max(1) == 5
    obs0, tape, ri, pid, _g, _g5 = synthetic_case(m, 'left', B, H, seed=1)
    tapes = candidate_tapes(m, tape, limit + 2, seed=1)
    with pytest.raises(ValueError) as e:                                   # over the limit: EB_EINVAL, the limit in the message
        m.t_cand_vjp(obs0, tapes, ri)
    assert '%d candidates' % (limit + 2) in str(e.value) and 'limit of %d' % limit in str(e.value)
    m.t_cand_vjp(obs0, tapes[:limit].contiguous(), ri)                     # at the limit it runs
    with pytest.raises(ValueError) as e:                                   # no gradient asked for: the value-only entry exists
        m.t_cand_vjp(obs0, tapes[:2].contiguous(), ri, g_tapes=False)
    assert 'eb_rollout_tape_cand' in str(e.value) and 'g_action_tapes' in str(e.value)
    with pytest.raises(ValueError):                                        # w5 is the cotangent: required
        m.t_cand_vjp(obs0, tapes[:2].contiguous(), ri, w5=None)
    for ld in (1, B - 1, -1):                                              # ref_ld between 1 and n_env - 1 (and negative)
        with pytest.raises(ValueError):
            m.t_cand_vjp(obs0, tapes[:2].contiguous(), ri.view(1, B).expand(2, B).contiguous(), ld)
    with pytest.raises(ValueError) as e:                                   # training mode without ref_idx
        m.t_cand_vjp(obs0, tapes[:2].contiguous(), None)
    assert 'ref_idx' in str(e.value)
    with pytest.raises(ValueError):                                        # horizon beyond 128
        m.t_cand_vjp(obs0, torch.zeros((1, 129, B, 2), device='cuda'), ri)
    with pytest.raises(ValueError):
        m.api.rollout_tape_cand_vjp_max(m.h, 129, C.byref(C.c_int32(0)))
    sel = CandGradModel('left', n_veh=8, n_future=0, mode='selecting')
    o8, t8, _ri, _pid, _g, _g5 = synthetic_case(sel, 'left', B, 5, seed=2)
    with pytest.raises(ValueError):                                        # a path id out of range in selecting mode
        sel.t_cand_vjp(o8, candidate_tapes(sel, t8, 2, seed=1), None, 0, [0, 3], 0)
    with pytest.raises(ValueError):
        sel.t_cand_vjp(o8, candidate_tapes(sel, t8, 2, seed=1), None, 0, None, 7)
    # n_env == 0 and n_cand == 0: no-ops that succeed
    m.api.rollout_tape_cand_vjp(m.h, 0, 3, 5, None, None, None, 0, None, 0, 0, None, None, None, None, None, m.stream)
    m.api.rollout_tape_cand_vjp(m.h, 8, 0, 5, None, None, None, 0, None, 0, 0, None, None, None, None, None, m.stream)
    # the facade evaluates a set beyond the limit in chunks: the bits of the per-chunk launches
    model = EnvironmentModel('left', 0, mode='training', n_veh=64)
    assert tape_cand_grad_max(model, H) == limit
    cost, g, out5, g_obs = rollout_tape_candidates_grad(model, obs0, tapes, WEIGHTS[0], ref_indexes=ri, want_out5=True, want_g_obs=True)
    assert out5.shape == (limit + 2, H, 5, B) and cost.shape == (limit + 2, B) and g.shape == tapes.shape and g_obs.shape == (limit + 2, B, 9)
    a = m.t_cand_vjp(obs0, tapes[:limit].contiguous(), ri)
    b = m.t_cand_vjp(obs0, tapes[limit:].contiguous(), ri)
    for got, x, y in zip((out5, cost, g_obs, g), a, b):
        assert same(got, torch.cat([x, y]))
    cost2, g2, none5, none0 = rollout_tape_candidates_grad(model, obs0, tapes, WEIGHTS[0], ref_indexes=ri)
    assert none5 is None and none0 is None and same(cost2, cost) and same(g2, g)
    with pytest.raises(_capi.EbError):                                     # fp16 state has no reverse pass
        rollout_tape_candidates_grad(EnvironmentModel('left', 0, mode='training', state_dtype='float16'), obs0, tapes, WEIGHTS[0])
    with pytest.raises(ValueError):
        rollout_tape_candidates_grad(model, obs0, tapes, None, ref_indexes=ri)
    with pytest.raises(ValueError):
        rollout_tape_candidates_grad(model, obs0, tapes[:, :, :5], WEIGHTS[0], ref_indexes=ri)


# ---- against the reference directly: G19 ----
RATIOS = {}


@pytest.mark.parametrize('task', TASKS)
def test_g19_gradients_of_the_three_paths_in_one_launch(task):
    """For every G19 row, the three paths as the three candidates of ONE launch (retrack: each candidate starts from the row's
    tracking error on its path): g_action_tapes at the zero tape and at the fixture's second tape point meet
    |g - g64| <= 4 E_c + 2^-20 max|g64| per column (tests/_grad_cases.py), cost at the zero tape matches J0[p] (the sanity tolerance
    of tests/test_gpu_mpc.py: rtol 1e-4, atol 1e-3).
    Measured on an MI355X, largest err / tolerance: left 0.27, straight 0.25, right 0.32 (G16's figure for eb_rollout_tape_vjp: 0.52)."""
    z = golden('g19_mpc_paths_%s' % task)
    g5 = golden('g5_rollout_%s_N%d_training_nf0' % (task, NATIVE[task]))
    m = CandGradModel(task, n_veh=NATIVE[task], n_future=0, mode='training', modes=[str(v) for v in g5['modes']])
    import torch
    B, H, P = len(z['rows']), int(z['horizon']), 3
    obs0 = m.to_dev(z['obs0'])
    ri = torch.arange(P, dtype=torch.int32, device='cuda').view(P, 1).expand(P, B).contiguous()
    worst = 0.0
    for tag, tapes in (('0', np.zeros((P, H, B, 2), np.float32)), ('2', z['tape2'].astype(np.float32))):
        _o5, J, _g0, gt = m.t_cand_vjp(obs0, m.to_dev(tapes), ri, B, None, 0, True, z['weights'])
        gt = gt.cpu().numpy()
        for p in range(P):
            got, ref = np.moveaxis(gt[p], 0, 1), np.moveaxis(z['g%s_act64' % tag][p], 0, 1)           # [B, H, 2]
            E, ok = z['E%s_act' % tag][p], z['ok%s' % tag][p]
            err = np.abs(got.astype(np.float64) - ref)[ok].max((0, 1))
            worst = max(worst, float((err / column_tolerance(E, ref, ok)).max()))
            check_columns(got, ref, E, ok, 'g19 %s path %d tape point %s' % (task, p, tag))
        if tag == '0':
            assert np.allclose(J.double().cpu().numpy(), z['J0'], rtol=1e-4, atol=1e-3)
    RATIOS[task] = worst
    print('g19 %s: largest err / tolerance over paths, tape points and columns: %.3f' % (task, worst))


# ---- the solver ----
def const_starts(H, B):
    """zero tape, constant (0, -1), constant (0, +1): steer 0 with full braking / full acceleration"""
    import torch
    U = torch.zeros((3, H, B, 2), device='cuda')
    U[1, :, :, 1], U[2, :, :, 1] = -1.0, 1.0
    return U


def independent_cost(model, mpc, rows, ref, u):
    """mpc.cost_from_out5 of an independent eb_rollout_tape over u from `rows`"""
    from env_build_amd.mpc import cost_from_out5
    model.reset(rows, ref)
    _final, out5 = model.rollout_tape(u)
    return cost_from_out5(out5.t if hasattr(out5, 't') else out5, mpc.weights)


@pytest.mark.parametrize('task', TASKS)
def test_solve_with_all_starts_on_the_g17_rows(task):
    import torch
    from env_build_amd.cand import tape_cand_grad_max
    from env_build_amd.mpc import first_minimum
    z, model, mpc, obs0, ref = mpc_setup(task)
    H, B = int(z['horizon']), obs0.shape[0]
    starts = const_starts(H, B)
    u, J, info = mpc.solve(obs0, ref_indexes=ref, u_init=starts, starts='all')
    iters = info['iterations']
    assert u.shape == (H, B, 2) and J.shape == (B,) and bool(torch.isfinite(J).all()) and float(u.abs().max()) <= 1.0
    assert same(J, independent_cost(model, mpc, obs0, ref, u))
    hist, Js, idx = info['J_history'], info['J_starts'], info['start_index']
    assert hist.shape == (iters + 1, 3, B) and Js.shape == (3, B) and idx.shape == (B,) and info['accepted'].shape == (iters, 3, B)
    assert bool((hist[1:] <= hist[:-1]).all()) and same(hist[-1], Js)
    assert torch.equal(idx, first_minimum(Js)) and same(J, Js.gather(0, idx.view(1, B))[0]) and same(J, Js.min(0).values)
    assert info['launches'] == mpc.launch_count(3, iters) == 1 + iters * (mpc.ls_trials + 1)
    limit = tape_cand_grad_max(model, H)
    assert limit >= 3
    for K in sorted({1, 2, 3, limit}):                                     # launches do not depend on K up to the limit
        UK = torch.cat([starts, starts])[:K].contiguous()
        _u, _J, i3 = mpc.solve(obs0, ref_indexes=ref, u_init=UK, starts='all', iterations=3)
        assert i3['launches'] == 1 + 3 * (mpc.ls_trials + 1) == mpc.launch_count(K, 3), K
    _u, _J, over = mpc.solve(obs0, ref_indexes=ref, u_init=torch.cat([starts, starts, starts])[:limit + 1].contiguous(), starts='all', iterations=2)
    assert over['launches'] == mpc.launch_count(limit + 1, 2) == 2 + 2 * (mpc.ls_trials + 2)    # two gradient chunks
    u2, J2, info2 = mpc.solve(obs0, ref_indexes=ref, u_init=starts, starts='all')
    assert same(u2, u) and same(J2, J) and same(info2['J_history'], hist)  # a second solve repeats its bits
    # the single-start solver from the same run, and whether start k of the K-start solve repeats the single-start solve from U[k]
    u1, J1, info1 = mpc.solve(obs0, ref_indexes=ref)
    equal = []
    for k in range(3):
        _uk, Jk, ik = mpc.solve(obs0, ref_indexes=ref, u_init=starts[k].contiguous())
        equal.append(same(Jk, Js[k]) and same(ik['J_history'], hist[:, k].contiguous()))
    print('g17 %s: start k of solve(starts="all") has the bits of the single-start solve from U[k]: %s' % (task, equal))
    assert all(equal)
    assert bool((J <= J1).all())                                           # start 0 is the zero tape: never worse than the single start
    Jh, Jd = J.double().cpu().numpy(), J1.double().cpu().numpy()
    multi, single = int((Jh > z['J_ref'] + 0.1).sum()), int((Jd > z['J_ref'] + 0.1).sum())
    print('g17 %s: %d of %d rows disagree with J_ref + 0.1 with three starts (single start from the same run: %d, reference alone: %d)'
          % (task, multi, B, single, int((~z['ref_alone_ok']).sum())))
    assert 4 * multi <= B
    with pytest.raises(ValueError):
        mpc.solve(obs0, ref_indexes=ref, starts='all')                     # needs K starts
    with pytest.raises(ValueError):
        mpc.solve(obs0, ref_indexes=ref, u_init=starts, starts='every')


def test_solve_with_all_starts_and_a_fused_line_search():
    """the K * ls_trials trial tapes of an iteration through launch_chunks: the bits of the unfused multi-start solve"""
    import torch
    from env_build_amd.cand import tape_cand_max
    from env_build_amd.mpc import OpenLoopMPC
    z, model, mpc, obs0, ref = mpc_setup('straight')
    H, B = int(z['horizon']), obs0.shape[0]
    fused = OpenLoopMPC(model, horizon=H, fused_line_search=True)
    starts = const_starts(H, B)
    u, J, info = mpc.solve(obs0, ref_indexes=ref, u_init=starts, starts='all', iterations=12)
    uf, Jf, inf = fused.solve(obs0, ref_indexes=ref, u_init=starts, starts='all', iterations=12)
    assert same(u, uf) and same(J, Jf) and same(info['J_history'], inf['J_history']) and torch.equal(info['accepted'], inf['accepted'])
    per_iter = -(-3 * fused.ls_trials // tape_cand_max(model, H)) + 1
    assert inf['launches'] == fused.launch_count(3, 12) == 1 + 12 * per_iter < info['launches']


@pytest.mark.parametrize('task', TASKS)
def test_solve_paths_on_the_g19_rows(task):
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.mpc import OpenLoopMPC, first_minimum
    z = golden('g19_mpc_paths_%s' % task)
    model = EnvironmentModel(task, 0, mode='training')
    H, B, P = int(z['horizon']), len(z['rows']), 3
    mpc = OpenLoopMPC(model, horizon=H)
    obs0 = torch.from_numpy(np.ascontiguousarray(z['obs0'])).to(model.device)
    u, J, info = mpc.solve_paths(obs0)
    iters = info['iterations']
    assert u.shape == (H, B, 2) and J.shape == (B,) and bool(torch.isfinite(J).all()) and float(u.abs().max()) <= 1.0
    Jp, Up, idx, hist = info['J_paths'], info['u_paths'], info['path_index'], info['J_history']
    assert Jp.shape == (P, B) and Up.shape == (P, H, B, 2) and idx.shape == (B,) and hist.shape == (iters + 1, P, B)
    for p in range(P):                                                     # J_paths[p]: the cost of u_paths[p] on the retracked row
        rp = torch.full((B,), p, dtype=torch.int32, device=model.device)
        rows = retracked_rows(model, obs0, 0, rp)
        assert same(Jp[p], independent_cost(model, mpc, rows, rp, Up[p].contiguous())), 'path %d' % p
    assert bool((hist[1:] <= hist[:-1]).all()) and same(hist[-1], Jp)
    assert torch.equal(idx, first_minimum(Jp)) and same(J, Jp.min(0).values)
    assert same(u, Up.gather(0, idx.view(1, 1, B, 1).expand(1, H, B, 2))[0])
    assert np.allclose(hist[0].double().cpu().numpy(), z['J0'], rtol=1e-4, atol=1e-3)
    assert info['launches'] == mpc.launch_count(P, iters) == 1 + iters * (mpc.ls_trials + 1)
    u2, J2, info2 = mpc.solve_paths(obs0)
    assert same(u2, u) and same(J2, J) and torch.equal(info2['path_index'], idx)
    Jh = J.double().cpu().numpy()
    agree = Jh <= z['Jbest_ref'] + 0.1
    ref_best = z['J_ref'].argmin(0)
    for r, jr, jh, a, b, ok in zip(z['rows'], z['J_ref'].T, Jp.double().cpu().numpy().T, ref_best, idx.cpu().numpy(), agree):
        print('g19 %-9s row %3d  SLSQP per path %s  MI355X per path %s  best path %d / %d  %s'
              % (task, r, np.round(jr, 3), np.round(jh, 3), a, b, 'agrees' if ok else 'DISAGREES'))
    print('g19 %s: %d of %d rows disagree with Jbest_ref + 0.1 (reference alone: %d, float64 projected gradient: %d); %d of %d rows pick '
          'the reference\'s best path' % (task, (~agree).sum(), B, (~z['ref_alone_ok']).sum(), (~z['pg64_ok']).sum(),
                                         int((ref_best == idx.cpu().numpy()).sum()), B))
    assert 4 * int((~agree).sum()) <= B


def test_solve_paths_in_selecting_mode():
    """path_ids instead of ref_idx [P, B]: the same invariants on a synthetic batch"""
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.mpc import OpenLoopMPC, cost_from_out5, first_minimum
    model = EnvironmentModel('left', 0, mode='selecting')
    tm = CandGradModel('left', n_veh=model.veh_num, n_future=0, mode='selecting')
    B, H = 150, 25
    obs0, _tape, _ri, _pid, _g, _g5 = synthetic_case(tm, 'left', B, H, seed=9)
    mpc = OpenLoopMPC(model, horizon=H, iterations=10)
    u, J, info = mpc.solve_paths(obs0)
    assert info['launches'] == 1 + 10 * 4 and torch.equal(info['path_index'], first_minimum(info['J_paths']))
    for p in range(3):
        model.ref_path.set_path(p)
        rows = retracked_rows(model, obs0, 0)
        f5, _ = tm.t_forward_tape(rows, info['u_paths'][p].contiguous(), None, p)
        assert same(info['J_paths'][p], cost_from_out5(f5, mpc.weights)), 'path %d' % p
    assert same(J, info['J_paths'].min(0).values) and bool((info['J_history'][1:] <= info['J_history'][:-1]).all())
    with pytest.raises(ValueError):
        mpc.solve_paths(obs0, u_init=torch.zeros((2, H, B, 2), device='cuda'))


def test_paths_example_runs_a_few_control_steps():
    mod = load_example('mpc_paths')
    r = mod.run(n_env=128, control_steps=3, iterations=8)
    import torch
    assert torch.isfinite(r['J_first']).all() and bool((r['J_first'] <= r['J0_first']).all())
    assert bool((r['J_first'] < r['J0_first']).any()) and torch.isfinite(r['reward_sum']).all() and torch.isfinite(r['J_last']).all()
    assert r['path_first'].shape == (128,) and int(r['path_last'].max()) <= 2
    assert r['launches'] == 3 * (1 + 8 * 4)                                # three paths: the launches of a single-start solve
