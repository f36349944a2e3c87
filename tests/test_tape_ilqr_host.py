"""CPU (-m "not gpu"): the iLQR family on the host (the ABI of include/envbuild_ilqr.h: tests/test_family_abi.py): the per-env text of the kernel
(csrc/eb_ilqr_device.h, compiled for the host) is driven over the CPU oracle's forward on the G17 start rows and on G18's edge chains:
  A, B, l_z, l_u   equal grad::env_vjp with unit cotangents numerically (+0 and -0 alike);
  l_zz, l_uu       within |v - v64| <= 4 E + 2^-20 max|v64| of ilqr.lq_reference in float64, E the restatement's own float32 run's
                   distance from its float64 run (the bound of tests/_grad_cases.py);
  k, K, dv         within the same bound of ilqr.riccati_reference in float64 on the SAME model, the (row, step) pairs excluded at
                   which the two precisions — or the code under test — take different active sets or fallbacks, and every earlier
                   step of such a row (the sweep runs backwards: what follows a different set is a different problem); at most 1 %.
The restatement of the feedback law is the header's bit for bit; the box QP meets a brute-force search; ILQRMPC's update rule
(mpc.ilqr_loop) reaches the known optimum of a toy LQ problem in one iteration at alpha = 1."""
import ctypes as C

import numpy as np
import pytest

from env_build_amd import _capi
from tests._helpers import HostModel, build_host_harness, golden, oracle_lib, _p
from tests._grad_cases import TASKS, MAX_EXCLUDED, edge_cases
from tests._tape import NATIVE, bound_check, diverged, same_numbers

W5 = np.array([-1.0, 10.0, 0.0, 0.0, 0.0], np.float32)
W5_ALL = np.array([-0.5, 3.0, 2.0, 0.25, 1.5], np.float32)          # every row of out5 carries weight


# ---- the kernel's per-env text on the host ----
@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    """tests/_ilqr_host_harness.hip: csrc/eb_ilqr_device.h compiled for the host, with the flags of the tape-gradient harness"""
    return build_host_harness(tmp_path_factory, '_ilqr_host_harness.hip', 'ilqr_host')


class Scene(object):
    def __init__(self, name, task, n_veh, n_future, mode, modes, obs0, tape, ref_idx, path_id):
        self.name, self.task, self.n_veh, self.n_future, self.mode, self.modes = name, task, n_veh, n_future, mode, modes
        self.obs0, self.tape, self.ref_idx, self.path_id = obs0, np.ascontiguousarray(tape, np.float32), ref_idx, path_id
        self.nd = 9 + 3 * n_future


_scene_cache = {}


def scenes(task):
    """the G17 start rows (the reference optimiser's tape as the tape) and G18's edge chains (walls, clip, crowded, remote), each with
    the pre-step obs of every step from the CPU oracle; computed once per task and shared"""
    if task in _scene_cache:
        return _scene_cache[task]
    z = golden('g17_mpc_%s' % task)
    g5 = golden('g5_rollout_%s_N%d_training_nf0' % (task, NATIVE[task]))
    rows = z['rows']
    out = [Scene('g17', task, NATIVE[task], 0, 'training', [str(v) for v in g5['modes']], g5['obs0'][rows], z['u_ref'],
                 g5['ref_idx'][rows].astype(np.int32), 0)]
    for c in edge_cases(task)[1]:
        out.append(Scene('g18 ' + c.name, task, c.n_veh, c.n_future, c.mode, None, c['obs0'], c['tape'], c.ref_idx(), c.path_id))
    for s in out:
        m = HostModel(oracle_lib(), task, n_veh=s.n_veh, n_future=s.n_future, mode=s.mode, modes=s.modes)
        obs, pre = s.obs0, []
        for a in s.tape:
            pre.append(obs)
            obs, _o5, _ = m.rollout_step(obs, a, s.ref_idx if s.mode == 'training' else None, s.path_id)
        s.pre = np.ascontiguousarray(np.stack(pre), np.float32)                 # [H, B, D]
        ri = s.ref_idx
        s.has_path = np.ascontiguousarray(((ri >= 0) & (ri < 3)) if s.mode == 'training' else np.ones(len(s.obs0), bool), dtype=np.int32)
    _scene_cache[task] = out
    return out


def host_ilqr(h, s, w5, mu=None):
    H, n, D = s.pre.shape
    lq, gains = np.full((H, 157, n), np.nan, np.float32), np.full((H, 14, n), np.nan, np.float32)
    dv, sets = np.full((2, n), np.nan, np.float32), np.full((H, n), -9, np.int32)
    w5 = np.ascontiguousarray(w5, np.float32)
    mu = None if mu is None else np.ascontiguousarray(mu, np.float32)
    h.host_ilqr(_capi.TASK_ID[s.task], n, H, D, s.nd, s.n_veh, _p(s.pre), _p(s.tape), _p(s.has_path), _p(w5), _p(mu), _p(lq), _p(gains),
                _p(dv), _p(sets))
    return lq, gains, dv, sets


@pytest.mark.parametrize('task', TASKS)
def test_quadratic_model_on_the_host(task, harness):
    from env_build_amd.ilqr import lq_reference, unpack_lq
    for s in scenes(task):
        for w5 in (W5, W5_ALL):
            H, n, D = s.pre.shape
            lq, _g, _dv, _sets = host_ilqr(harness, s, w5)
            M = unpack_lq(lq)
            # A, B, l_z, l_u against grad::env_vjp with unit cotangents
            rows = np.full((H, 10, 11, n), np.nan, np.float32)
            harness.host_vjp_rows(_capi.TASK_ID[task], n, H, D, s.nd, s.n_veh, _p(s.pre), _p(s.tape), _p(s.has_path),
                                  _p(np.ascontiguousarray(w5, np.float32)), _p(rows))
            rows = np.moveaxis(rows, 3, 1)                                      # [H, n, 10, 11]
            assert same_numbers(M['A'], rows[:, :, :9, :9]) and same_numbers(M['B'], rows[:, :, :9, 9:]), s.name
            assert same_numbers(M['l_z'], rows[:, :, 9, :9]) and same_numbers(M['l_u'], rows[:, :, 9, 9:]), s.name
            assert not M['A'][:, :, :, 6:].any(), 'columns 6..8 of A are zero'
            assert np.isfinite(lq).all()
            # l_zz, l_uu against the restatement
            flat = s.pre.reshape(H * n, D)
            act = s.tape.reshape(H * n, 2)
            z32, u32 = lq_reference(task, flat, act, w5, s.nd, np.float32)
            z64, u64 = lq_reference(task, flat, act, w5, s.nd, np.float64)
            iu = np.triu_indices(9)
            keep = np.ones(H * n, bool)
            bound_check(M['l_zz'].reshape(H * n, 9, 9)[:, iu[0], iu[1]], z32[:, iu[0], iu[1]], z64[:, iu[0], iu[1]], keep,
                        'host l_zz %s %s' % (task, s.name))
            bound_check(M['l_uu'].reshape(H * n, 2), u32, u64, keep, 'host l_uu %s %s' % (task, s.name))
            # positive semi-definite by construction
            assert np.linalg.eigvalsh(M['l_zz'].astype(np.float64)).min() >= -1e-4 * max(1.0, float(np.abs(M['l_zz']).max()))


@pytest.mark.parametrize('task', TASKS)
def test_backward_sweep_on_the_host(task, harness):
    from env_build_amd.ilqr import riccati_reference, unpack_lq
    pairs = excluded = alone = 0
    seen = set()
    for i, s in enumerate(scenes(task)):
        H, n, _D = s.pre.shape
        mu = None if i % 2 == 0 else np.linspace(0.0, 2.0, n).astype(np.float32)
        lq, gains, dv, sets = host_ilqr(harness, s, W5, mu)
        M = unpack_lq(lq)
        args = (M['A'], M['B'], M['l_z'], M['l_u'], M['l_zz'], M['l_uu'], s.tape, mu)
        g32, dv32, s32 = riccati_reference(*args, dtype=np.float32)
        g64, dv64, s64 = riccati_reference(*args, dtype=np.float64)
        bad_alone = diverged(s32, s64)
        bad = bad_alone | diverged(sets, s64)
        pairs += H * n; excluded += int(bad.sum()); alone += int(bad_alone.sum())
        seen |= set(np.unique(sets[~bad]).tolist())
        assert np.isfinite(gains).all() and np.isfinite(dv).all()
        keep = ~bad
        assert keep.any()
        bound_check(np.moveaxis(gains, 1, 2), np.moveaxis(g32, 1, 2), np.moveaxis(g64, 1, 2), keep, 'host gains %s %s' % (task, s.name))
        row_ok = keep.all(0)
        if row_ok.any():
            bound_check(dv.T, dv32.T, dv64.T, row_ok, 'host dv %s %s' % (task, s.name))
            assert (dv[0][row_ok] <= 0).all() and (dv[1][row_ok] >= 0).all()     # a descent direction of a convex model
        # u + k stays in the box (to rounding) wherever u is in it
        moved = np.moveaxis(s.tape, 2, 1) + gains[:, 0:2]
        assert (np.abs(moved)[np.abs(np.moveaxis(s.tape, 2, 1)) <= 1] <= 1 + 1e-5).all()
    print('host sweep %s: %d of %d (row, step) pairs excluded (the restatement alone: %d); active sets seen: %s'
          % (task, excluded, pairs, alone, sorted(seen)))
    assert alone <= MAX_EXCLUDED * pairs, 'the restatement alone exceeds the cap on these scenes'
    assert excluded <= MAX_EXCLUDED * pairs
    assert 0 in seen and len(seen) >= 2, 'the scenes reach the free set and at least one clamped set'


def test_closed_form_on_a_free_straight_row(harness):
    """straight task, a row with no near record and no active wall: l_zz = -2 w5[0] diag of the reward's constants on columns 2, 6, 7, 8
    and zero elsewhere"""
    from env_build_amd.ilqr import unpack_lq
    s = scenes('straight')[0]
    H, n, D = s.pre.shape
    lq, _g, _dv, _s = host_ilqr(harness, s, W5_ALL)
    M = unpack_lq(lq)
    o = s.pre.astype(np.float64)
    veh = o[:, :, s.nd:].reshape(H, n, s.n_veh, 4)
    far = (np.hypot(o[:, :, 3, None] - veh[..., 0], o[:, :, 4, None] - veh[..., 1]) > 8.0).all(2)
    mid = (np.abs(o[:, :, 4]) < 20.0)                                           # inside the junction: no wall condition holds
    free = far & mid
    assert free.sum() >= 10
    want = np.zeros((9, 9))
    c = 2.0 * 0.5
    want[2, 2], want[6, 6], want[7, 7], want[8, 8] = c * 0.02, c * 0.8, c * 30.0 * (np.pi / 180.0) ** 2, c * 0.05
    got = M['l_zz'][free].astype(np.float64)
    assert np.abs(got - want).max() <= 2.0 ** -20
    assert not got[:, 3:6, 3:6].any()
    assert np.allclose(M['l_uu'][free], [c * 5 * 0.16, c * 0.05 * 2.25 ** 2], rtol=1e-6)


def test_feedback_restatement_is_the_header_bit_for_bit(harness):
    from env_build_amd.ilqr import feedback_actions_reference
    rng = np.random.default_rng(5)
    H, n = 7, 13
    u_nom = rng.uniform(-1.3, 1.3, (H, n, 2)).astype(np.float32)
    x = rng.normal(0, 5, (H, 6, n)).astype(np.float32)
    x_nom = (x + rng.normal(0, 0.3, (H, 6, n))).astype(np.float32)
    gains = rng.normal(0, 0.4, (H, 14, n)).astype(np.float32)
    u_nom[2, 3, 0] = np.nan
    for alpha in (1.0, 0.3, 0.015625):
        got = np.full((H, n, 2), 7.0, np.float32)
        harness.host_feedback(n, H, C.c_float(alpha), _p(u_nom), _p(x), _p(x_nom), _p(gains), _p(got))
        want = feedback_actions_reference(u_nom, x, x_nom, gains, alpha)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.isnan(got[2, 3, 0]) and np.nanmax(np.abs(got)) <= 1.0 and (np.abs(got) == 1.0).any() and (np.abs(got) < 1.0).any()
    assert np.array_equal(feedback_actions_reference(u_nom, None, None, None, None).view(np.uint32), np.clip(u_nom, -1, 1).view(np.uint32))


def test_box_qp_meets_a_brute_force_search(harness):
    """2 000 random positive definite problems (a third with the unconstrained optimum inside the box): the enumeration's answer has
    the lowest objective of a dense grid over the box, and every active set is reached"""
    from env_build_amd.ilqr import _box_qp
    rng = np.random.default_rng(2)
    n = 2000
    L = rng.normal(0, 1, (n, 2, 2))
    Q = (L @ np.swapaxes(L, 1, 2) + 0.05 * np.eye(2)).astype(np.float32)
    g = (rng.normal(0, 2, (n, 2)) * rng.choice([0.2, 1.0, 4.0], (n, 1))).astype(np.float32)
    u = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    lo, hi = (-1 - u).astype(np.float32), (1 - u).astype(np.float32)
    d, st = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
    q3 = np.ascontiguousarray(np.stack([Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 1]], 1))
    harness.host_box_qp(n, _p(q3), _p(g), _p(lo), _p(hi), _p(d), _p(st))
    assert set(st.tolist()) == set(range(9))
    d64, _free, st64 = _box_qp(Q.astype(np.float64), g.astype(np.float64), lo.astype(np.float64), hi.astype(np.float64))
    agree = st == st64
    assert agree.mean() > 0.99 and np.abs(d[agree] - d64[agree]).max() < 1e-4
    f = lambda v: 0.5 * np.einsum('ni,nij,nj->n', v, Q.astype(np.float64), v) + (g * v).sum(1)
    best = f(d.astype(np.float64))
    grid = np.linspace(0, 1, 41)
    for a in grid:
        for b in grid:
            v = np.stack([lo[:, 0] + a * (hi[:, 0] - lo[:, 0]), lo[:, 1] + b * (hi[:, 1] - lo[:, 1])], 1).astype(np.float64)
            assert (best <= f(v) + 1e-4 * (1 + np.abs(best))).all()
    assert (d >= lo - 1e-6).all() and (d <= hi + 1e-6).all()


def test_ilqr_loop_reaches_the_optimum_of_a_toy_lq_problem_in_one_iteration():
    """z' = A z + B u, cost sum_t 1/2 (z_t - m_t)^T C (z_t - m_t) + 1/2 r |u_t|^2: the Gauss-Newton model is exact, so ONE iteration at
    alpha = 1 lands on the optimum.  Env 0: A = 0, B = (I; 0) — every step is a box QP of its own and the optimum is a clip; env 1: a
    coupled A with targets small enough for the box to stay inactive — the optimum is the solution of the normal equations."""
    import torch
    from env_build_amd.ilqr import riccati_reference
    from env_build_amd.mpc import ilqr_loop
    rng = np.random.default_rng(0)
    H, B, r = 6, 2, 0.3
    A = np.zeros((B, 9, 9)); Bm = np.zeros((B, 9, 2))
    Bm[0, 0, 0] = Bm[0, 1, 1] = 1.0
    A[1, :6, :6] = 0.6 * rng.normal(0, 0.4, (6, 6)) + 0.3 * np.eye(6)
    Bm[1, :6] = rng.normal(0, 1, (6, 2))
    Cm = np.diag([3.0, 2.0, 1.0, 0.5, 0.2, 0.1, 0.0, 0.0, 0.0])
    m = rng.normal(0, 1, (H + 1, B, 9)); m[:, 0] *= 2.0; m[:, 1] *= 0.05; m[:, :, 6:] = 0.0
    z0 = np.zeros((B, 9))
    alphas = (1.0, 0.5)
    calls = []

    def roll(u_of):                                                              # u_of(t, z) -> u_t;  -> (J, u, z_pre)
        z, J, us, zs = z0.copy(), np.zeros(B), [], []
        for t in range(H):
            u = u_of(t, z)
            J += 0.5 * np.einsum('bi,ij,bj->b', z - m[t], Cm, z - m[t]) + 0.5 * r * (u * u).sum(1)
            us.append(u); zs.append(z)
            z = np.einsum('bij,bj->bi', A, z) + np.einsum('bij,bj->bi', Bm, u)
        J += 0.5 * np.einsum('bi,ij,bj->b', z - m[H], Cm, z - m[H])
        return J, np.stack(us), np.stack(zs)

    def step(u_nom, x_nom, gains, mu, need_gains):
        calls.append(need_gains)
        u_nom = u_nom.numpy()
        cands = [roll(lambda t, z: np.clip(u_nom[t], -1, 1))]
        if gains is not None:
            g, xn = gains.numpy(), x_nom.numpy()
            for al in alphas:
                def law(t, z, al=al):
                    k, K = g[t, 0:2].T, np.stack([g[t, 2:8].T, g[t, 8:14].T], 1)          # [B, 2], [B, 2, 6]
                    return np.clip(u_nom[t] + al * k + np.einsum('bac,bc->ba', K, z[:, :6] - xn[t].T), -1, 1)
                cands.append(roll(law))
        J = np.stack([c[0] for c in cands])
        idx = J.argmin(0)
        u = np.stack([cands[idx[b]][1][:, b] for b in range(B)], 1)
        z = np.stack([cands[idx[b]][2][:, b] for b in range(B)], 1)                      # [H, B, 9]
        # the exact model along (z, u); the final cost folds into the last step's successor: V_H(z) = 1/2 (z - m_H)^T C (z - m_H), which
        # riccati_reference (V_H = 0) gets as an extra step with B = 0 and zero control cost
        Hs = H + 1
        AA, BB = np.broadcast_to(A, (Hs, B, 9, 9)).copy(), np.broadcast_to(Bm, (Hs, B, 9, 2)).copy()
        BB[H] = 0.0
        zz = np.concatenate([z, (np.einsum('bij,bj->bi', A, z[-1]) + np.einsum('bij,bj->bi', Bm, u[-1]))[None]])
        uu = np.concatenate([u, np.zeros((1, B, 2))])
        lz, lu = np.einsum('ij,hbj->hbi', Cm, zz - m), r * uu
        luu = np.full((Hs, B, 2), r); luu[H] = 1.0
        gn, _dv, _sets = riccati_reference(AA, BB, lz, lu, np.broadcast_to(Cm, (Hs, B, 9, 9)), luu, uu,
                                           None if mu is None else mu.numpy(), dtype=np.float64)
        t = torch.from_numpy
        return dict(best_index=t(idx.astype(np.int32)), best_cost=t(J[idx, np.arange(B)]), u=t(u), x=t(np.moveaxis(z[:, :, :6], 1, 2).copy()),
                    gains=t(gn[:H].copy()))
    u, J, info = ilqr_loop(step, torch.zeros((H, B, 2), dtype=torch.float64), 2)
    u = u.numpy()
    # env 0: separable — u_t = clip(c m_{t+1} / (c + r)) per component
    c = np.array([3.0, 2.0])
    want0 = np.clip(c * m[1:, 0, :2] / (c + r), -1, 1)
    assert np.abs(u[:, 0] - want0).max() < 1e-9 and (np.abs(want0) == 1).any() and (np.abs(want0) < 1).any()
    # env 1: the normal equations of the unconstrained problem
    n_u = 2 * H
    def J1(v):
        return roll(lambda t, z: np.stack([np.zeros(2), v[2 * t:2 * t + 2]]))[0][1]
    g0 = np.array([(J1(e) - J1(-e)) / 2 for e in np.eye(n_u)])                  # exact for a quadratic
    Hm = np.array([[(J1(a + b) - J1(a) - J1(b) + J1(np.zeros(n_u))) for b in np.eye(n_u)] for a in np.eye(n_u)])
    want1 = np.linalg.solve(Hm, -g0).reshape(H, 2)
    assert np.abs(want1).max() < 1 and np.abs(u[:, 1] - want1).max() < 1e-8
    hist = info['J_history'].numpy()
    assert hist.shape == (3, B) and (hist[1:] <= hist[:-1] + 1e-12).all() and (hist[1] < hist[0]).all()
    assert info['best_index'][0].tolist() == [1, 1], 'alpha = 1 wins the first iteration'
    assert abs(hist[2] - hist[1]).max() < 1e-9, 'one iteration was enough'
    assert info['mu'].shape == (B,) and float(info['mu'].max()) <= 1e-3
    assert calls == [True, True, False], 'the last call is told that nobody reads its gains'


def test_mu_schedule_of_the_loop():
    """candidate 0 wins: mu -> max(10 mu, 1e-3) capped at 1e6; else mu -> 0.2 mu, flushed to 0 below 1e-6"""
    import torch
    from env_build_amd.mpc import ilqr_loop
    picks = iter([[0, 1, 0, 1], [0, 1, 0, 1], [1, 0, 1, 1]])
    seen = []

    def step(u_nom, x_nom, gains, mu, need_gains):
        seen.append(None if mu is None else mu.clone())
        idx = torch.zeros(4, dtype=torch.int32) if gains is None else torch.tensor(next(picks), dtype=torch.int32)
        return dict(best_index=idx, best_cost=torch.zeros(4), u=u_nom, x=torch.zeros(1), gains=torch.zeros(1))
    _u, _J, info = ilqr_loop(step, torch.zeros((1, 4, 2)), 3, mu0=2e-6)
    assert seen[0] is None and torch.allclose(seen[1], torch.full((4,), 2e-6))
    assert torch.allclose(seen[2], torch.tensor([1e-3, 0.0, 1e-3, 0.0]))        # 0.2 * 2e-6 < 1e-6: flushed
    assert torch.allclose(seen[3], torch.tensor([1e-2, 0.0, 1e-2, 0.0]))
    assert torch.allclose(info['mu'], torch.tensor([2e-3, 1e-3, 2e-3, 0.0]))
    big = ilqr_loop(lambda u, x, g, mu, need: dict(best_index=torch.zeros(1, dtype=torch.int32), best_cost=torch.zeros(1), u=u, x=u, gains=u),
                    torch.zeros((1, 1, 2)), 12, mu0=1.0)[2]['mu']
    assert float(big) == 1e6
