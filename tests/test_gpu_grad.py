"""GPU (-m gpu): the reverse pass of the rollout step (include/envbuild_grad.h, csrc/eb_rollout_vjp.hip) against the gradient
fixtures of scripts/gen_golden_grad.py (G15, G16 and the edge scenes of G18) — the reference's own Python under autograd, float64 —
and its invariants; the autograd façade (env_build_amd/grad.py) against the manual chain of C calls; the ADP example.

Tolerance and the cap on excluded rows: tests/_grad_cases.py.  Every check prints max |g - g64| / E per column before it asserts."""
import numpy as np
import pytest

from env_build_amd import _capi
from tests._helpers import DeviceModel
from tests._grad_cases import TASKS, MAX_EXCLUDED, cases, check_columns, edge_cases
from tests._tape import load_example

pytestmark = pytest.mark.gpu


class GradModel(DeviceModel):
    """DeviceModel + the two entries of include/envbuild_grad.h, NumPy in / NumPy out"""

    def step_vjp(self, obs, actions, ref_idx, path_id, g_obs_out, g_out5, full=False):
        ob, ac, ri = self._in(obs), self._in(actions), self._in(ref_idx, np.int32)
        go, g5 = self._in(g_obs_out), self._in(g_out5)
        n, nd = len(ob), self.D - 4 * self.n_veh
        ld_in = self.D if full else nd
        gi, ga = self._out((n, ld_in)), self._out((n, 2))
        gi.fill_(float('nan')); ga.fill_(float('nan'))
        self.api.rollout_step_vjp(self.h, n, self._ptr(ob), self._ptr(ac), self._ptr(ri), int(path_id), self._ptr(go),
                                  0 if go is None else go.shape[1], self._ptr(g5), self._ptr(gi), ld_in, self._ptr(ga), self.stream)
        return self._ret(gi), self._ret(ga)

    def chain_vjp(self, obs_steps, tape, ref_idx, path_id, g_obs_final, g_out5_steps):
        ob, tp, ri = self._in(obs_steps), self._in(tape), self._in(ref_idx, np.int32)
        gf, g5 = self._in(g_obs_final), self._in(g_out5_steps)
        H, n, nd = tp.shape[0], tp.shape[1], self.D - 4 * self.n_veh
        work, g0, gt = self._out((n, nd)), self._out((n, nd)), self._out((H, n, 2))
        self.api.rollout_chain_vjp(self.h, n, H, self._ptr(ob), self._ptr(tp), self._ptr(ri), int(path_id), self._ptr(gf),
                                   0 if gf is None else gf.shape[1], self._ptr(g5), self._ptr(work), self._ptr(g0), self._ptr(gt),
                                   self.stream)
        return self._ret(g0), self._ret(gt)


def model_for(task, c):
    return GradModel(task, n_veh=c.n_veh, n_future=c.n_future, mode=c.mode)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def step_cases_meet_the_reference(task, cs, tag):
    rows = sum(len(c['ok']) for c in cs)
    assert sum(int((~c['ok']).sum()) for c in cs) <= MAX_EXCLUDED * rows
    for c in cs:
        m = model_for(task, c)
        gi, ga = m.step_vjp(c['obs'], c['actions'], c.ref_idx(), c.path_id, c['g_obs_out'], c['g_out5'])
        check_columns(gi, c['g_obs64'], c['E_obs'], c['ok'], '%s %s %s obs' % (tag, task, c.name))
        check_columns(ga, c['g_act64'], c['E_act'], c['ok'], '%s %s %s act' % (tag, task, c.name))
        full, ga2 = m.step_vjp(c['obs'], c['actions'], c.ref_idx(), c.path_id, c['g_obs_out'], c['g_out5'], full=True)
        assert same_bits(full[:, :c.nd], gi) and same_bits(ga2, ga)          # ld_in == D: the same bits ...
        assert not full[:, c.nd:].any() and not np.signbit(full[:, c.nd:]).any()   # ... and +0 in every vehicle column


@pytest.mark.parametrize('task', TASKS)
def test_step_vjp_meets_the_reference_gradients(task):
    """g15: single steps.  |g - g64| <= 4 E_c + 2^-20 max|g64| per column over the flagged rows; at most 1 % of the rows excluded."""
    step_cases_meet_the_reference(task, cases('g15_grad_step', task), 'g15')


@pytest.mark.parametrize('task', TASKS)
def test_step_vjp_meets_the_edge_scenes(task):
    """g18: every wall condition by either circle, every two2one region, both sides of the v_x clip, crowded and empty
    neighbourhoods at 32 and 64 slots, egos off the cell grid — the same bound, both row forms."""
    step_cases_meet_the_reference(task, edge_cases(task)[0], 'g18')


def forward_states(m, c):
    """the package's own forward: pre-step obs of every step [H, B, D] and out5 [H, 5, B]"""
    obs, pre, out5 = c['obs0'], [], []
    for a in c['tape']:
        pre.append(obs)
        obs, o5, _ = m.rollout_step(obs, a, c.ref_idx(), c.path_id)
        out5.append(o5)
    return np.stack(pre), np.stack(out5)


def chain_cases_meet_the_reference(task, cs, tag):
    rows = excluded = 0
    for c in cs:
        m = model_for(task, c)
        pre, out5 = forward_states(m, c)
        want = c['out5_f32'].astype(np.float64)
        ok = c['ok'] & (np.abs(out5 - want) <= 5e-6 + 1e-5 * np.abs(want)).all((0, 1))
        rows += len(ok); excluded += int((~ok).sum())
        g0, gt = m.chain_vjp(pre, c['tape'], c.ref_idx(), c.path_id, c['g_obs_final'], c['g_out5_steps'])
        g_next, gts = c['g_obs_final'], [None] * len(pre)
        for t in reversed(range(len(pre))):
            g_next, gts[t] = m.step_vjp(pre[t], c['tape'][t], c.ref_idx(), c.path_id, g_next, c['g_out5_steps'][t])
        assert same_bits(g_next, g0) and same_bits(np.stack(gts), gt), c.name
        check_columns(g0, c['g_obs64'], c['E_obs'], ok, '%s %s %s obs0' % (tag, task, c.name))
        check_columns(np.moveaxis(gt, 0, 1), np.moveaxis(c['g_act64'], 0, 1), c['E_act'], ok, '%s %s %s tape' % (tag, task, c.name))
    print('%s %s: %d of %d rows excluded' % (tag, task, excluded, rows))
    assert excluded <= MAX_EXCLUDED * rows


@pytest.mark.parametrize('task', TASKS)
def test_chain_vjp_meets_the_reference_gradients(task):
    """g16: chains of 5 and 25 steps through eb_rollout_chain_vjp and through a loop of eb_rollout_step_vjp (same bits).  The
    forward states are the package's own; a row whose forward out5 leaves the fixture's float32 forward by more than the tolerance
    reference-generated fixtures are held to here (rtol 1e-5 next to atol 5e-6) counts as excluded, under the same 1 % cap."""
    chain_cases_meet_the_reference(task, cases('g16_grad_chain', task), 'g16')


@pytest.mark.parametrize('task', TASKS)
def test_chain_vjp_meets_the_edge_chains(task):
    """g18: a 25-step chain from the junction's exit side and a 5-step one at 32 slots from next to the entry lane's walls, held as
    the g16 chains are (the 1 % cap over this file's chain rows)."""
    chain_cases_meet_the_reference(task, edge_cases(task)[1], 'g18')


def test_null_cotangents_are_zero_arrays():
    c = cases('g15_grad_step', 'left')[1]          # native slots, two look-ahead points
    m = model_for('left', c)
    args = (c['obs'], c['actions'], c.ref_idx(), c.path_id)
    z_obs, z_5 = np.zeros_like(c['g_obs_out']), np.zeros_like(c['g_out5'])
    for go, g5, go0, g50 in ((None, c['g_out5'], z_obs, c['g_out5']), (c['g_obs_out'], None, c['g_obs_out'], z_5), (None, None, z_obs, z_5)):
        a, b = m.step_vjp(*args, go, g5), m.step_vjp(*args, go0, g50)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # (== : a -0 of one side is a +0 of the other)
    a = m.step_vjp(*args, None, None)
    assert not a[0].any() and not a[1].any()


def test_clips_block_the_gradient_exactly():
    """actions beyond +-1.05 (DAM:129) and a v_x the clip to [0, 35] changed (DAM:390) get exact zeros"""
    c = cases('g15_grad_step', 'straight')[0]
    m = model_for('straight', c)
    obs, act = c['obs'].copy(), c['actions'].copy()
    act[0::4, 0] = 1.2; act[1::4, 1] = -1.06; act[2::4] = (-3.0, 1.0500001)
    gi, ga = m.step_vjp(obs, act, c.ref_idx(), c.path_id, c['g_obs_out'], c['g_out5'])
    assert not ga[0::4, 0].any() and not ga[1::4, 1].any() and not ga[2::4].any()
    assert ga[0::4, 1].all() and ga[1::4, 0].all() and ga[3::4].all()
    # v_x: rows braking from a crawl end below 0, rows near 35 m/s accelerating end above: only the g_obs_out[:, 0] and the
    # tracking-speed cotangent (column 8) reach the pre-clip v_x, so with every other cotangent zero the whole gradient is zero
    obs[0::2, 0] = 0.05; act[0::2, 1] = -1.0; obs[1::2, 0] = 34.99; act[1::2, 1] = 1.0
    obs[:, 1:3] = 0.0
    g = np.zeros_like(c['g_obs_out']); g[:, 0] = 1.0; g[:, 8] = 2.0
    gi, ga = m.step_vjp(obs, act, c.ref_idx(), c.path_id, g, None)
    assert not gi.any() and not ga.any()
    obs[:, 0] = 5.0                                   # the same rows unclipped: the cotangent arrives
    gi, ga = m.step_vjp(obs, act, c.ref_idx(), c.path_id, g, None)
    assert (gi[:, 0] == 3.0).all() and ga[:, 1].all()


def test_rows_without_a_path_have_no_tracking_gradient():
    c = [c for c in cases('g15_grad_step', 'left') if 'synth' in c.name][0]
    ri = c['ref_idx']
    off = (ri < 0) | (ri > 2)
    assert off.sum() >= 6 and c.mode == 'training'
    m = model_for('left', c)
    g2 = c['g_obs_out'].copy(); g2[:, 6:] += 1.0      # other cotangents on every tracking column of the NEXT obs
    a = m.step_vjp(c['obs'], c['actions'], ri, 0, c['g_obs_out'], c['g_out5'])
    b = m.step_vjp(c['obs'], c['actions'], ri, 0, g2, c['g_out5'])
    assert same_bits(a[0][off], b[0][off]) and same_bits(a[1][off], b[1][off])
    assert (a[0][~off] != b[0][~off]).any(1).all()


def test_batch_sizes_and_position_independence():
    c = cases('g15_grad_step', 'right')[0]
    m = model_for('right', c)
    full = m.step_vjp(c['obs'], c['actions'], c.ref_idx(), c.path_id, c['g_obs_out'], c['g_out5'])
    ri = c.ref_idx()
    for n, first in ((1, 0), (1, 77), (63, 5), (257 - 1, 0)):
        s = slice(first, first + n)
        got = m.step_vjp(c['obs'][s], c['actions'][s], None if ri is None else ri[s], c.path_id, c['g_obs_out'][s], c['g_out5'][:, s])
        assert same_bits(got[0], full[0][s]) and same_bits(got[1], full[1][s]), (n, first)
    idx = np.arange(257) % len(c['obs'])              # 257 rows: a last block with one env
    got = m.step_vjp(c['obs'][idx], c['actions'][idx], None if ri is None else ri[idx], c.path_id, c['g_obs_out'][idx], c['g_out5'][:, idx])
    assert same_bits(got[0], full[0][idx]) and same_bits(got[1], full[1][idx])
    # n_env == 0: a no-op that succeeds
    m.api.rollout_step_vjp(m.h, 0, None, None, None, 0, None, 0, None, None, c.nd, None, m.stream)
    with pytest.raises(ValueError):                   # ld_in is nd or D
        m.api.rollout_step_vjp(m.h, 1, *(m._ptr(m._in(np.zeros((1, m.D)))),) * 2, m._ptr(m._in(np.zeros(1), np.int32)), 0, None, 0, None,
                               m._ptr(m._out((1, m.D))), c.nd + 1, m._ptr(m._out((1, 2))), m.stream)


def test_training_mode_needs_ref_idx():
    c = cases('g15_grad_step', 'left')[0]
    assert c.mode == 'training'
    m = model_for('left', c)
    with pytest.raises(ValueError) as e:
        m.step_vjp(c['obs'], c['actions'], None, 0, c['g_obs_out'], c['g_out5'])
    assert 'ref_idx' in str(e.value)


def test_large_batch_has_the_bits_of_the_small_one_and_repeats_them():
    """the fixture rows tiled to 65 536 envs x 32 slots: every row the bits of the small-batch run, and again on a second run"""
    c = [c for c in cases('g15_grad_step', 'left') if c.n_veh == 32 and c.mode == 'training'][0]
    m = model_for('left', c)
    small = m.step_vjp(c['obs'], c['actions'], c.ref_idx(), c.path_id, c['g_obs_out'], c['g_out5'], full=True)
    idx = np.arange(65536) % len(c['obs'])
    args = (c['obs'][idx], c['actions'][idx], c['ref_idx'][idx], c.path_id, c['g_obs_out'][idx], np.ascontiguousarray(c['g_out5'][:, idx]))
    big = m.step_vjp(*args, full=True)
    assert same_bits(big[0], small[0][idx]) and same_bits(big[1], small[1][idx])
    again = m.step_vjp(*args, full=True)
    assert same_bits(again[0], big[0]) and same_bits(again[1], big[1])


@pytest.mark.parametrize('task,mode', [('left', 'training'), ('right', 'selecting')])
def test_autograd_through_a_policy_loop_equals_the_manual_chain(task, mode):
    import torch
    from env_build_amd.grad import DifferentiableEnvironmentModel
    from env_build_amd.dynamics_and_models import EnvironmentModel, DevArray
    ex = load_example('adp_policy_gradient')
    H, B = 5, 96
    dm = DifferentiableEnvironmentModel(task, 0, mode=mode, n_veh=16)
    obs0, ref = ex.start_states(dm, B, seed=3)
    policy = ex.make_policy(dm.obs_dim, dm.device, hidden=32, seed=1)
    scale = torch.full((dm.obs_dim,), 0.05, device=dm.device)
    w5 = torch.tensor([-1.0, 10.0, 0.5, 0.25, 2.0], device=dm.device)

    def start(model, o):
        if mode == 'training':
            model.reset(o, ref)
        else:
            model.add_traj(o, 1)

    # autograd
    o = obs0.clone().requires_grad_(True)
    start(dm, o)
    obs, loss, outs = o, 0.0, []
    for _ in range(H):
        r = dm.rollout_out(policy(obs * scale))
        obs = r[0]
        outs.append(torch.stack(r[1:]))
        loss = loss + (outs[-1] * w5[:, None]).sum()
    loss = loss + obs[:, :9].sum()
    grads = torch.autograd.grad(loss, [o] + list(policy.parameters()))
    assert grads[0][:, :9].abs().sum() > 0 and all(torch.isfinite(g).all() for g in grads)
    # the model alone (constant actions): the vehicle columns of d loss / d obses are exactly zero (stop_gradient)
    o2 = obs0.clone().requires_grad_(True)
    start(dm, o2)
    r = dm.rollout_out(torch.zeros((B, 2), device=dm.device))
    g2, = torch.autograd.grad(r[0].sum() + sum(v.sum() for v in r[1:]), [o2])
    assert not g2[:, 9:].any() and g2[:, :9].abs().sum() > 0

    # EnvironmentModel (no graph) is untouched: DevArrays, the same forward bits
    em = EnvironmentModel(task, 0, mode=mode, n_veh=16)
    start(em, obs0)
    with torch.no_grad():
        x, pre, acts = obs0, [], []
        for t in range(H):
            a = policy(x * scale)
            pre.append(x); acts.append(a)
            r = em.rollout_out(a)
            assert all(type(v) is DevArray or isinstance(v, DevArray) for v in r) and not r[0].t.requires_grad
            assert torch.equal(torch.stack([v.t for v in r[1:]]), outs[t].detach())
            x = r[0].t
        assert torch.equal(x, obs.detach())

    # the manual chain: eb_rollout_step_vjp per step, the policy's own backward in between
    api, nd, D = dm.api, 9, dm.obs_dim
    g_next = torch.zeros((B, D), device=dm.device); g_next[:, :9] = 1.0
    g5 = w5[:, None].expand(5, B).contiguous()
    gp = [torch.zeros_like(p) for p in policy.parameters()]
    ri = dm._ref_idx_dev if mode == 'training' else None
    st = torch.cuda.current_stream().cuda_stream
    for t in reversed(range(H)):
        g_obs, g_act = torch.empty((B, D), device=dm.device), torch.empty((B, 2), device=dm.device)
        api.rollout_step_vjp(dm.handle, B, pre[t].data_ptr(), acts[t].data_ptr(), None if ri is None else ri.data_ptr(), 1,
                             g_next.data_ptr(), D, g5.data_ptr(), g_obs.data_ptr(), D, g_act.data_ptr(), st)
        xin = pre[t].clone().requires_grad_(True)
        back = torch.autograd.grad(policy(xin * scale), [xin] + list(policy.parameters()), g_act)
        g_next = g_obs + back[0]
        for acc, g in zip(gp, back[1:]):
            acc += g
    assert torch.allclose(g_next, grads[0], rtol=1e-5, atol=1e-6 * float(grads[0].abs().max()))
    for a, b in zip(gp, grads[1:]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))


def test_differentiable_model_refuses_what_has_no_reverse_pass():
    from env_build_amd.grad import DifferentiableEnvironmentModel
    with pytest.raises(_capi.EbError):
        DifferentiableEnvironmentModel('left', state_dtype='float16')
    dm = DifferentiableEnvironmentModel('left')
    with pytest.raises(_capi.EbError):
        dm.rollout_tape(np.zeros((2, 4, 2), np.float32))


def test_adp_example_runs_one_training_step():
    r = load_example('adp_policy_gradient').run(n_env=512, horizon=25, iterations=2)
    assert len(r['losses']) == 2 and all(np.isfinite(r['losses']))
    assert np.isfinite(r['grad_norm']) and r['grad_norm'] > 0.0
