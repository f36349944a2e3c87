"""-m gpu: the HIP library against the CPU oracle, call-for-call through the same C-ABI, on seeded
inputs; plus the golden fixtures replayed on the GPU.

Bars:
  * every state/obs float, index and mask: BIT-EXACT against the oracle (the deterministic
    sin/cos/atan kernels and -ffp-contract=off make that possible);
  * the four penalty sums (punish_term_for_training, real_punish_term, veh2veh4real and the two
    veh2veh dict entries): rtol 1e-6 — the kernel adds each vehicle's 4-term partial to the running
    sum (vehicle order preserved) instead of the reference's term-by-term running sum, a
    re-association worth <= a few ulp; north_star's bar is rtol 1e-5;
  * against the reference-generated golden fixtures: rtol 1e-5 + atol 5e-6 (ulp-level sin/cos
    differences between NumPy and our kernels, accumulated over 25 closed-loop steps; the observed
    excess over the rtol term is printed under "parity margins" at the end of the run).
"""
import glob
import os

import numpy as np
import pytest

from env_build_amd.synthetic import assemble_obs, make_rollout_inputs
from env_build_amd.endtoend_env_utils import VEH_NUM
from tests._helpers import (GOLDEN, DeviceModel, HostModel, bits_equal, check_out5, close, golden, initial_obs, oracle_lib,
                            record_host)

pytestmark = pytest.mark.gpu
TASKS = ('left', 'straight', 'right')
FIX_ATOL = 5e-6    # next to rtol 1e-5 against reference-generated fixtures (tests/test_oracle_golden.py: ATOL)


def _pair(task, **kw):
    """the oracle, its penalty sums in the kernels' order (so that they are compared bit for bit), and the device"""
    return HostModel(oracle_lib(), task, penalty_order='record', **kw), DeviceModel(task, **kw)


_initial_obs = initial_obs      # (tests/_helpers.py: the census rows are held to the same text)


def _check_out5(o5_d, o5_h, where):
    check_out5(o5_d, o5_h, where, exact=True)


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('n_veh', ['native', 16, 32, 64])
@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_rollout_25_steps_bit_exact(task, n_veh, mode):
    N = VEH_NUM[task] if n_veh == 'native' else n_veh
    B, H = 1000, 25          # not a multiple of the envs-per-block tile: exercises the ragged tail
    host, dev = _pair(task, n_veh=N, mode=mode)
    inp = make_rollout_inputs(task, B, N, H, seed=11 + N)
    if mode == 'selecting':
        inp['ref_idx'][:] = 2
    obs_h = obs_d = _initial_obs(host, inp)
    for t in range(H):
        obs_h, o5_h, sc_h = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'], 2)
        obs_d, o5_d, sc_d = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'], 2)
        assert np.array_equal(sc_d, sc_h)
        bad = np.argwhere(obs_d != obs_h)
        assert bad.size == 0, 'step %d: %d obs words differ, first %s' % (t, len(bad), bad[:4].tolist())
        _check_out5(o5_d, o5_h, 'step %d' % t)


@pytest.mark.parametrize('tile', [0, 1, 2])
@pytest.mark.parametrize('task,N', [('left', 32), ('straight', 9), ('right', 64), ('left', 16), ('right', 5)])
def test_every_tile_shape_computes_the_same_bits(task, N, tile):
    """The headline tile (2048 records) is only picked by batch size from 32 768 envs up; force each tile
    shape on a small ragged batch (slot counts that do and do not divide the record lanes)."""
    B, H = 777, 6
    host, dev = _pair(task, n_veh=N)
    dev.set_tile(tile)
    inp = make_rollout_inputs(task, B, N, H, seed=100 + N + tile)
    obs_h = obs_d = _initial_obs(host, inp)
    for t in range(H):
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        assert np.array_equal(obs_d, obs_h), 'step %d' % t
        _check_out5(o5_d, o5_h, 'step %d' % t)
    nxt = dev.compute_next_obses(obs_d, inp['actions'][0] * 0.3, inp['ref_idx'])   # the no-reward form of the kernel
    assert np.array_equal(nxt, host.compute_next_obses(obs_h, inp['actions'][0] * 0.3, inp['ref_idx']))


@pytest.mark.parametrize('rolling,by_progress', [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('task,N,B', [('left', 32, 777), ('straight', 9, 1500), ('right', 64, 333), ('left', 16, 8200)])
def test_every_launch_schedule_computes_the_same_bits(task, N, B, rolling, by_progress):
    """Round 6: the 2048-record tile's two scheduling choices — every record load up front or three in flight per lane with the next
    one requested as a record is done; the hardware's oldest-first issue or a priority that falls as a wave advances — are picked by the
    grid's size (eb_capi.hip:rollout_sched) and change WHEN things happen, never what is computed: each combination forced on ragged
    batches (slot counts that do and do not divide the record lanes, more than one block per CU at 8 200 envs), against the oracle."""
    H = 4
    host, dev = _pair(task, n_veh=N)
    dev.set_tile(0)
    dev.set_rollout_sched(rolling, by_progress)
    inp = make_rollout_inputs(task, B, N, H, seed=300 + N + 2 * rolling + by_progress)
    obs_h = obs_d = _initial_obs(host, inp)
    for t in range(H):
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        assert np.array_equal(obs_d, obs_h), 'step %d' % t
        _check_out5(o5_d, o5_h, 'step %d' % t)
    nxt = dev.compute_next_obses(obs_d, inp['actions'][0] * 0.3, inp['ref_idx'])   # the no-reward form of the kernel
    assert np.array_equal(nxt, host.compute_next_obses(obs_h, inp['actions'][0] * 0.3, inp['ref_idx']))
    with pytest.raises(ValueError):
        dev.set_rollout_sched(2, 0)


def test_rollout_launch_plan_follows_the_measured_rules():
    """eb_debug_rollout_plan: the tile shape and launch schedule eb_rollout_step takes by itself (eb_capi.hip:pick_variant /
    rollout_sched; the sweeps behind the rules: profiles/r6_sched_sweep*.txt, r6_tile_sweep2.txt).  Stated for the MI355X's 256 CUs."""
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip('the expectations below are for 256 CUs')
    d32, d16, d64, d9 = (DeviceModel('left', n_veh=32), DeviceModel('left', n_veh=16), DeviceModel('left', n_veh=64),
                         DeviceModel('straight', n_veh=9))
    assert d32.rollout_plan(65536) == (0, 1024, 0, 1)        # the headline: every load up front, priority by progress
    assert d32.rollout_plan(32768) == (0, 512, 1, 1)         # two tiles per CU: rolling loads
    assert d32.rollout_plan(49152) == (0, 768, 1, 1) and d32.rollout_plan(262144) == (0, 4096, 0, 1)
    assert d32.rollout_plan(16384) == (1, 512, 0, 1) and d32.rollout_plan(4096)[0] == 2
    assert d64.rollout_plan(65536) == (0, 2048, 1, 1)        # 32-env tiles: rolling at any size
    assert d16.rollout_plan(65536) == (1, 1024, 0, 1)        # at most 16 slots: the 1024-record tile
    assert d9.rollout_plan(65536)[0] == 1 and d16.rollout_plan(4096) == (2, 256, 0, 0)
    d32.set_rollout_sched(0, 0)
    assert d32.rollout_plan(32768) == (0, 512, 0, 0)
    d32.set_tile(1)
    assert d32.rollout_plan(32768)[0] == 1
    import ctypes
    host = HostModel(oracle_lib(), 'left', n_veh=32)
    with pytest.raises(ValueError):                          # the CPU library launches nothing
        host.api.debug_rollout_plan(host.h, 100, (ctypes.c_int32 * 4)())


@pytest.mark.parametrize('tile,sched', [(0, (-1, -1)), (0, (0, 0)), (0, (1, 1)), (2, (-1, -1))])
@pytest.mark.parametrize('N', [32, 9])
def test_crowded_and_remote_scenes(N, tile, sched):
    """Edge scenes of the penalty path and the closest-point search:
       * every vehicle within a few metres of the ego -> every record is queued (the queue drains mid-tile);
       * egos far outside the closest-point cell grid (and on its border) -> the pruned full search;
       * stopped vehicles, zero / tiny headings and speeds -> the exact-division fallback."""
    task, B = 'left', 300
    host, dev = _pair(task, n_veh=N)
    dev.set_tile(tile)
    dev.set_rollout_sched(*sched)
    inp = make_rollout_inputs(task, B, N, 4, seed=77)
    rng = np.random.default_rng(5)
    veh = inp['veh'].reshape(B, N, 4).copy()
    ego = inp['ego'].copy()
    veh[:100, :, 0] = ego[:100, None, 3] + rng.uniform(-4, 4, (100, N))      # crowded
    veh[:100, :, 1] = ego[:100, None, 4] + rng.uniform(-4, 4, (100, N))
    ego[100:150, 3] = rng.uniform(-400, 400, 50)                                # remote egos
    ego[100:150, 4] = rng.uniform(-400, 400, 50)
    ego[150:160, 3] = np.float32(-75.0) + np.arange(10, dtype=np.float32) * np.float32(1e-6)   # grid border
    veh[160:200, :, 2] = 0.0                                                     # stopped
    veh[200:220, :, 3] = 0.0
    veh[220:240, :, 3] = np.float32(1e-38)
    veh[240:260, :, 2] = np.float32(3e-39)                                       # denormal speed
    veh[260:280, :, 3] = -0.0
    veh[280:290, :, 0:2] = rng.uniform(-20, 20, (10, N, 2))                        # stopped in the junction, heading -0.0:
    veh[280:290, :, 2] = 0.0                                                     # the right-turn slots give -0 / 10 -> -0
    veh[280:290, :, 3] = -0.0
    veh[290:294, :, 2] = np.inf                                                  # non-finite records: inf - inf -> NaN
    veh[294:297, :, 3] = -np.inf
    veh[297:300, :, 3] = np.float32(2e38)                                        # phi * pi overflows
    inp['ego'], inp['veh'] = ego, veh.reshape(B, 4 * N)
    obs_h = obs_d = _initial_obs(host, inp)
    for t in range(4):
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        nan_h, nan_d = np.isnan(obs_h), np.isnan(obs_d)                         # NaN payloads are the FPU's business
        assert np.array_equal(nan_h, nan_d), 'step %d' % t
        assert np.array_equal(obs_d.view(np.uint32)[~nan_h], obs_h.view(np.uint32)[~nan_h]), 'step %d' % t
        ok = ~np.isnan(o5_h).any(0)
        assert np.array_equal(ok, ~np.isnan(o5_d).any(0))
        _check_out5(o5_d[:, ok], o5_h[:, ok], 'step %d' % t)
        if t == 0:
            assert (o5_d[1][:100] > 0).all()     # the crowded envs do touch the 3.5 m margin


def test_configs1_exact_size_25_steps_bit_exact():
    """BASELINE configs[1] at its stated size: N_env = 4096, N_veh = 16, horizon 25 — every env against the oracle, per
    step and through the one-launch tape, the hipGraph plan and the episodic summary."""
    task, B, N, H = 'left', 4096, 16, 25
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=1)
    obs0 = _initial_obs(host, inp)
    obs_h = obs_d = obs0
    o5_all = []
    for t in range(H):
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        assert np.array_equal(obs_d, obs_h), 'step %d' % t
        _check_out5(o5_d, o5_h, 'step %d' % t)
        o5_all.append(o5_d)
    tape_obs, tape_o5 = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(tape_obs, obs_d) and np.array_equal(tape_o5, np.stack(o5_all))
    plan_obs, plan_o5, s8 = dev.plan_run(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(plan_obs, obs_d) and np.array_equal(plan_o5, tape_o5)
    assert s8[6] == B and s8[7] == H and abs(s8[0] - tape_o5[:, 0].astype(np.float64).sum()) <= 1e-6 * abs(s8[0])


def test_headline_size_against_oracle_on_sampled_envs():
    """BASELINE configs[2] (65 536 envs x 32 vehicles, the 2048-record tile chosen by batch size): envs are
    independent, so the oracle replays a sample of rows (first / last tile, tile borders, random rows) and
    must agree bit for bit; plus size-independent properties of the whole batch."""
    task, B, N, H = 'left', 65536, 32, 25
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=0)
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([np.arange(0, 130), np.arange(B - 130, B), np.arange(63, B, 4096), np.arange(64, B, 4096),
                                     rng.integers(0, B, 600)]))
    ego, ref = inp['ego'], inp['ref_idx']
    trk = host.tracking_error(ego[rows, 3], ego[rows, 4], ego[rows, 5], ego[rows, 0], 0, ref_idx=ref[rows])
    obs_d = assemble_obs(ego, np.zeros((B, 3), np.float32), inp['veh'])
    obs_d[rows, 6:9] = trk
    obs_h = obs_d[rows].copy()
    for t in range(H):
        obs_prev = obs_d
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], ref)
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t][rows], ref[rows])
        assert np.array_equal(obs_d[rows], obs_h), 'step %d' % t
        _check_out5(o5_d[:, rows], o5_h, 'step %d' % t)
        # whole batch: vehicle speed is carried over unchanged (DAM:422), headings stay in (-180, 180] (DAM:424-426),
        # penalties are non-negative sums of squares, nothing is NaN
        v_in, v_out = obs_prev[:, 9:].reshape(B, N, 4), obs_d[:, 9:].reshape(B, N, 4)
        assert np.array_equal(v_in[:, :, 2], v_out[:, :, 2])
        assert (v_out[:, :, 3] > -180.001).all() and (v_out[:, :, 3] <= 180.001).all()
        assert np.isfinite(obs_d).all() and np.isfinite(o5_d).all()
        assert (o5_d[1:] >= 0).all() and (o5_d[0] <= 0).all()
        assert (o5_d[1] >= o5_d[2] - 1e-6).all()          # the 3.5 m training margin dominates the 2.5 m real one


def test_headline_size_every_row_against_oracle():
    """BASELINE configs[2] in full — 65 536 envs x 32 vehicles x 25 closed-loop steps, EVERY row: per-step launches on the GPU against
    the oracle's tape (the oracle runs its rows on all host cores; a second or two)."""
    task, B, N, H = 'left', 65536, 32, 25
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=3)
    obs0 = _initial_obs(host, inp)
    out_h, o5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    obs_d = obs0
    for t in range(H):
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        _check_out5(o5_d, o5_h[t], 'step %d' % t)
    assert np.array_equal(obs_d, out_h)


def test_configs3_size_every_row_against_oracle():
    """BASELINE configs[3]'s whole batch on one GPU — 262 144 envs x 32 vehicles, 6 closed-loop steps, EVERY row (the multi-GPU job
    shards exactly these rows: sharding.shard_range), and the shards' episodic summaries folded against the whole batch's."""
    from env_build_amd.sharding import shard_range
    task, B, N, H = 'left', 262144, 32, 6
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=13)
    obs0 = _initial_obs(host, inp)
    out_h, o5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    out_d, o5_d = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(out_d, out_h)
    for t in range(H):
        _check_out5(o5_d[t], o5_h[t], 'step %d' % t)
    # 8 shards of 32 768 rows, each through its own call, are the same rows
    whole = dev.episode_summary(o5_d, out_d)
    parts = []
    for r in range(8):
        lo, hi = shard_range(B, r, 8)
        out_s, o5_s = dev.rollout_tape(obs0[lo:hi], inp['actions'][:, lo:hi], inp['ref_idx'][lo:hi])
        assert np.array_equal(out_s, out_d[lo:hi]) and np.array_equal(o5_s, o5_d[:, :, lo:hi])
        parts.append(dev.episode_summary(o5_s, out_s))
    parts = np.array(parts, np.float64)
    np.testing.assert_allclose(parts[:, 0:5].sum(0), whole[0:5], rtol=1e-6)
    assert parts[:, 5].max() == whole[5] and parts[:, 6].sum() == B


@pytest.mark.parametrize('task', TASKS)
def test_rollout_future_points_and_bad_ref_index(task):
    N, B = 8, 333
    host, dev = _pair(task, n_veh=N, n_future=3)
    inp = make_rollout_inputs(task, B, N, 6, seed=5, n_future=3)
    inp['ref_idx'][::7] = 5       # out-of-range path id -> tracking columns stay zero (DAM:342, 352)
    inp['ref_idx'][3::11] = -1
    obs_h = obs_d = _initial_obs(host, inp)
    for t in range(6):
        obs_h, o5_h, _ = host.rollout_step(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, _ = dev.rollout_step(obs_d, inp['actions'][t], inp['ref_idx'])
        assert np.array_equal(obs_d, obs_h)
        _check_out5(o5_d, o5_h, 'step %d' % t)
    assert np.all(obs_d[::7, 6:6 + 12] == 0)


def test_rollout_tape_equals_stepwise_and_oracle():
    task, N, B, H = 'left', 16, 513, 25
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=3)
    obs0 = _initial_obs(host, inp)
    out_h, o5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    out_d, o5_d = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(out_d, out_h)
    bits_equal(o5_d, o5_h, 'out5 of every step')
    for H2 in (1, 2):   # ping-pong parity of the output buffer
        a, _ = dev.rollout_tape(obs0, inp['actions'][:H2], inp['ref_idx'])
        b, _ = host.rollout_tape(obs0, inp['actions'][:H2], inp['ref_idx'])
        assert np.array_equal(a, b)


@pytest.mark.parametrize('task,N,B,H', [('left', 32, 2049, 25), ('right', 5, 100, 3), ('straight', 64, 777, 7)])
def test_plan_graph_replay_and_summary(task, N, B, H):
    """hipGraph-captured rollout (eb_plan_*) == eb_rollout_tape == the oracle; the episodic summary
    matches the oracle's float64 sums."""
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=21)
    obs0 = _initial_obs(host, inp)
    out_h, o5_h, s8_h = host.plan_run(obs0, inp['actions'], inp['ref_idx'])
    out_d, o5_d, s8_d = dev.plan_run(obs0, inp['actions'], inp['ref_idx'], replays=3)
    out_t, o5_t = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(out_d, out_h) and np.array_equal(out_d, out_t)
    assert np.array_equal(o5_d, o5_t)
    bits_equal(o5_d, o5_h, 'out5 of every step')
    # summary of the DEVICE's own out5 against the oracle's float64 reduction of the same numbers
    s8_ref = host.episode_summary(o5_d, out_d)
    np.testing.assert_allclose(s8_d, s8_ref, rtol=1e-6, atol=0)
    assert s8_d[3] == s8_ref[3] and s8_d[5] == s8_ref[5] and s8_d[6] == B and s8_d[7] == H
    np.testing.assert_allclose(s8_d, s8_h, rtol=1e-5, atol=0)
    assert np.array_equal(dev.episode_summary(o5_d, out_d), s8_d)


@pytest.mark.parametrize('task,N,B,H,tile', [('left', 32, 2049, 25, -1), ('left', 32, 2049, 3, 0), ('left', 32, 130, 2, 1),
                                             ('right', 5, 100, 3, -1), ('right', 5, 1, 1, -1), ('straight', 64, 777, 7, 2),
                                             ('straight', 9, 4097, 4, 0), ('left', 16, 40000, 5, -1)])
def test_accumulating_rollout_equals_the_two_pass_summary(task, N, B, H, tile):
    """ABI 5: the episodic summary collected by the rollout launches themselves (eb_rollout_step_acc: per-block float64 records,
    DPP wave reduction, a step's record made by the next step's launch; eb_episode_acc_finish: one fold) — same rows and outputs
    as eb_rollout_step bit for bit, the 8 floats of eb_episode_summary over the same out5 (sums rtol 1e-6, count and maximum equal),
    at every tile shape, ragged last tiles, one-step rollouts, twice in a row in one workspace (nothing is read from it), and through
    the plan's two forms."""
    host, dev = _pair(task, n_veh=N)
    if tile >= 0:
        dev.set_tile(tile)
    inp = make_rollout_inputs(task, B, N, H, seed=31 + B)
    obs0 = _initial_obs(host, inp)
    out_t, o5_t = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    want = host.episode_summary(o5_t, out_t)
    acc = dev.acc_workspace(B, H)
    for _ in range(2):
        out_d, o5_d, s8 = dev.rollout_acc(obs0, inp['actions'], inp['ref_idx'], acc=acc)
        assert np.array_equal(out_d, out_t) and np.array_equal(o5_d, o5_t)
        np.testing.assert_allclose(s8, want, rtol=1e-6, atol=0)
        assert s8[3] == want[3] and s8[5] == want[5] and s8[6] == B and s8[7] == H
    assert np.array_equal(dev.episode_summary(o5_t, out_t)[[3, 5, 6, 7]], s8[[3, 5, 6, 7]])
    for caller_acc in (True, 'finish'):
        out_p, o5_p, s8_p = dev.plan_run(obs0, inp['actions'], inp['ref_idx'], replays=2, caller_acc=caller_acc)
        assert np.array_equal(out_p, out_t) and np.array_equal(o5_p, o5_t) and np.array_equal(s8_p, s8)
    # against the oracle's own accumulating form
    _, _, s8_h = host.rollout_acc(obs0, inp['actions'], inp['ref_idx'])
    np.testing.assert_allclose(s8, s8_h, rtol=1e-5, atol=0)


def test_facade_binds_a_bare_cuda_device_at_construction():
    """A handle lives on one device: a model / env / policy built with a bare 'cuda' is bound to the device current at construction
    (explicit index), which is also whose current stream orders its launches — not whatever device is current at call time."""
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel, _resolve_device
    assert _resolve_device('cuda') == torch.device('cuda', torch.cuda.current_device())
    assert _resolve_device(torch.device('cuda', 0)).index == 0 and _resolve_device(None).index is not None
    m = EnvironmentModel('left', device='cuda')
    assert m.device.index == torch.cuda.current_device() and m._dev_index == m.device.index


def test_accumulating_rollout_is_tied_to_the_grid_of_its_first_step():
    """The records of an accumulating rollout are indexed by the launch grid: the step-0 launch fixes grid, batch and horizon for its
    workspace.  A tile shape forced between two steps is refused (EB_EINVAL, nothing launched); one forced between the last step and
    the fold does not move the fold off the records (it folds with the recorded grid); a fold asked for another batch is refused."""
    host, dev = _pair('left', n_veh=32)
    B, H = 5000, 3
    inp = make_rollout_inputs('left', B, 32, H, seed=77)
    obs0 = _initial_obs(host, inp)
    dev.set_tile(1)
    out_t, o5_t = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    want = dev.episode_summary(o5_t, out_t)
    ob, tp, ri = dev._in(obs0), dev._in(inp['actions']), dev._in(inp['ref_idx'], np.int32)
    bufs, out5, s8 = [dev._out(ob.shape), dev._out(ob.shape)], dev._out((H, 5, B)), dev._out((8,))
    acc = dev.acc_workspace(B, H)

    def step(t, cur, dst):
        dev.api.rollout_step_acc(dev.h, B, dev._ptr(cur), dev._ptr(tp[t]), dev._ptr(ri), 0, dev._ptr(dst), dev._ptr(out5[t]), None,
                                 dev._ptr(acc), t, H, dev._ptr(out5[t - 1]) if t else None, dev.stream)
    step(0, ob, bufs[0])
    dev.set_tile(2)                                  # another grid: the next step's records would land elsewhere
    with pytest.raises(ValueError):                  # (EB_EINVAL)
        step(1, bufs[0], bufs[1])
    dev.set_tile(1)
    step(1, bufs[0], bufs[1])
    step(2, bufs[1], bufs[0])
    dev.set_tile(2)                                  # ... and the fold still reads the records where the launches put them
    dev.api.episode_acc_finish(dev.h, B, H, dev._ptr(acc), dev._ptr(s8), dev.stream)
    got = dev._ret(s8)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert got[3] == want[3] and got[5] == want[5] and got[6] == B and got[7] == H
    assert np.array_equal(dev._ret(bufs[0]), out_t) and np.array_equal(dev._ret(out5), o5_t)
    with pytest.raises(ValueError):
        dev.api.episode_acc_finish(dev.h, B - 1, H, dev._ptr(acc), dev._ptr(s8), dev.stream)
    dev.set_tile(-1)


def test_accumulating_rollout_ignores_nan_rows_in_the_maximum():
    """a row whose delta_y is not a number never becomes the maximum (as in eb_episode_summary), the sum carries it"""
    host, dev = _pair('left', n_veh=8)
    inp = make_rollout_inputs('left', 200, 8, 2, seed=2)
    obs0 = _initial_obs(host, inp)
    obs0[17, 3] = np.nan                                   # ego x: the tracking error of the next obs is NaN
    out_t, o5_t = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.isnan(out_t[17, 6])
    want = host.episode_summary(o5_t, out_t)
    _, _, s8 = dev.rollout_acc(obs0, inp['actions'], inp['ref_idx'])
    assert s8[5] == want[5] and np.isfinite(s8[5]) and np.isnan(s8[4]) and np.isnan(want[4]) and s8[3] == want[3]


@pytest.mark.parametrize('B,H', [(1, 1), (3, 5), (255, 4), (256, 25), (257, 3), (1000, 25), (1001, 7), (65536, 25), (65536 + 260, 2)])
def test_episode_summary_sizes(B, H):
    """eb_episode_summary against the oracle's float64 sums at ragged sizes — fewer envs than a block, more than the grid covers
    in one pass — and twice in a row on the same handle (the partials of the first call are scratch)."""
    host, dev = _pair('left', n_veh=4)
    rng = np.random.default_rng(B + H)
    o5 = (rng.random((H, 5, B), dtype=np.float32) - np.float32(0.4)) * np.float32(3.0)
    o5[:, 2][rng.random((H, B)) < 0.9] = 0.0                      # punish_real: zero most of the time
    obs = rng.normal(size=(B, 6 + 3 + 4 * 4)).astype(np.float32)                 # task left, 4 slots, no future points: D = 25
    want = host.episode_summary(o5, obs)
    for _ in range(2):
        got = dev.episode_summary(o5, obs)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
        assert got[3] == want[3] and got[5] == want[5] and got[6] == B and got[7] == H


def test_event_marks_measure_stream_time():
    import ctypes as C
    host, dev = _pair('left', n_veh=32)
    inp = make_rollout_inputs('left', 8192, 32, 2, seed=1)
    obs0 = _initial_obs(host, inp)
    e0, e1 = C.c_void_p(), C.c_void_p()
    dev.api.event_create(dev.h, C.byref(e0)); dev.api.event_create(dev.h, C.byref(e1))
    dev.api.event_record(e0, dev.stream)
    for _ in range(20):
        dev.rollout_step(obs0, inp['actions'][0], inp['ref_idx'])
    dev.api.event_record(e1, dev.stream)
    ms = C.c_float()
    dev.api.event_elapsed_ms(e0, e1, C.byref(ms))
    assert 0.0 < ms.value < 5000.0
    dev.api.event_destroy(e0); dev.api.event_destroy(e1)


@pytest.mark.parametrize('task', TASKS)
def test_single_ops_bit_exact(task):
    N = VEH_NUM[task]
    host, dev = _pair(task, n_veh=N)
    rng = np.random.default_rng(8)
    n = 4099
    st = np.stack([rng.uniform(0, 12, n), rng.normal(0, .5, n), rng.normal(0, .3, n), rng.uniform(-60, 60, n),
                   rng.uniform(-60, 60, n), rng.uniform(-400, 400, n)], 1).astype(np.float32)
    st[:16, 0] = 0
    ac = np.stack([rng.uniform(-.42, .42, n), rng.uniform(-3.2, 1.7, n)], 1).astype(np.float32)
    for tau in (0.1, 0.05):
        (a, b), (c, d) = host.f_xu(st, ac, tau), dev.f_xu(st, ac, tau)
        assert np.array_equal(a, c) and np.array_equal(b, d)
    raw = rng.uniform(-1.3, 1.3, (n, 2)).astype(np.float32)
    assert np.array_equal(host.action_transform(raw), dev.action_transform(raw))
    inp = make_rollout_inputs(task, n, N, 1, seed=4)
    obs = _initial_obs(host, inp)
    (h5, h16), (d5, d16) = host.compute_rewards(obs, ac), dev.compute_rewards(obs, ac)
    _check_out5(d5, h5, 'compute_rewards')
    exact = [i for i in range(16) if i not in (12, 14)]
    assert np.array_equal(d16[exact], h16[exact])
    bits_equal(d16[[12, 14]], h16[[12, 14]], 'veh2veh4training / veh2veh4real of the dictionary')
    assert np.array_equal(host.compute_next_obses(obs, ac, inp['ref_idx']), dev.compute_next_obses(obs, ac, inp['ref_idx']))
    veh = inp['veh']
    assert np.array_equal(host.veh_predict(veh), dev.veh_predict(veh))
    x, y = rng.uniform(-70, 70, n).astype(np.float32), rng.uniform(-70, 70, n).astype(np.float32)
    phi, v = rng.uniform(-500, 500, n).astype(np.float32), rng.uniform(0, 12, n).astype(np.float32)
    for k in range(3):
        (hi, hp), (di, dp) = host.find_closest_point(x, y, path_id=k), dev.find_closest_point(x, y, path_id=k)
        assert np.array_equal(hi, di) and np.array_equal(hp, dp)
        for nf in (0, 4):
            assert np.array_equal(host.tracking_error(x, y, phi, v, nf, path_id=k), dev.tracking_error(x, y, phi, v, nf, path_id=k))
    ri = rng.integers(-1, 4, n).astype(np.int32)
    assert np.array_equal(host.tracking_error(x, y, phi, v, 1, ref_idx=ri), dev.tracking_error(x, y, phi, v, 1, ref_idx=ri))
    raw = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    np.testing.assert_array_equal(host.ss(obs, raw, inp['ref_idx'], 0, 0.1), dev.ss(obs, raw, inp['ref_idx'], 0, 0.1))


def test_empty_batch_and_errors():
    host, dev = _pair('left')
    z = np.zeros((0, dev.D), np.float32)
    out, o5, _ = dev.rollout_step(z, np.zeros((0, 2), np.float32), np.zeros((0,), np.int32))
    assert out.shape == (0, dev.D) and o5.shape == (5, 0)
    with pytest.raises(ValueError):   # training mode without ref_indexes
        dev.rollout_step(np.zeros((4, dev.D), np.float32), np.zeros((4, 2), np.float32), None)


@pytest.mark.parametrize('name', sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, 'g5_*.npz'))))
def test_golden_rollouts_on_gpu(name):
    _, _, task, N, mode, nf = name.split('_')
    g = golden(name)
    dev = DeviceModel(task, n_veh=int(N[1:]), n_future=int(nf[2:]), mode=mode, modes=[str(m) for m in g['modes']])
    obs, keep = g['obs0'], list(g['obs_step_index'])
    for t in range(g['actions'].shape[0]):
        obs, o5, _ = dev.rollout_step(obs, g['actions'][t], g['ref_idx'], 1)
        close(o5, g['out5'][t], 1e-5, FIX_ATOL, 'GPU G5 closed loop x25: out5')
        if t in keep:
            close(obs, g['obs_steps'][keep.index(t)], 1e-5, FIX_ATOL, 'GPU G5 closed loop x25: obs')


# ---- env-side kernels (endtoend.py): eb_env_ego_step / eb_get_obs / eb_judge_done -------------------------
from env_build_amd import _capi  # noqa: E402
from env_build_amd.endtoend_env_utils import VEHICLE_MODE_LIST  # noqa: E402


@pytest.mark.parametrize('task', TASKS)
def test_g6_env_logic_on_gpu(task):
    """The reference-generated env-logic fixture (filter / sort / pad, the seven done outcomes, collision hits
    and misses) replayed on the GPU: integer masks and copied floats bit-exact."""
    g = golden('g6_env_logic_%s' % task)
    dev = DeviceModel(task, mode='training')
    light_flag = ((g['v_light'] != 0) | (g['virtual'] != 0)).astype(np.uint8)
    obs = dev.get_obs(g['ego'], g['cand'], g['cand_mode'], light_flag, ref_idx=g['ref_index'])
    assert np.array_equal(obs[:, :6], g['obs'][:, :6])
    close(obs[:, 6:9], g['obs'][:, 6:9], 1e-5, FIX_ATOL, 'GPU G6 tracking columns')
    assert np.array_equal(obs[:, 9:], g['obs'][:, 9:])
    done = dev.judge_done(g['ego'], g['params'], g['obs'], g['cand'], g['cand_mode'], g['cand_lw'], g['v_light'])
    assert np.array_equal(done, g['done_code'])
    assert np.array_equal(done == 1, g['collision'] != 0)


@pytest.mark.parametrize('task', TASKS)
def test_g6_ego_dynamics_on_gpu(task):
    """a15: eb_ego_dynamics on the GPU — the device functions judge_bits runs (ego_r_bound, ego_corner) — equals the oracle bit for
    bit and the reference's own `_get_ego_dynamics` outputs (fixture G6: r_bound, Corner_point) within north_star's tolerance;
    the batched facade hands the same values out."""
    g = golden('g6_env_logic_%s' % task)
    host, dev = _pair(task)
    got, want = dev.ego_dynamics(g['ego'], g['params']), host.ego_dynamics(g['ego'], g['params'])
    assert np.array_equal(got, want)
    close(got[:, 2], g['r_bound'], 1e-5, 0.0, 'GPU G6 _get_ego_dynamics r_bound')
    close(got[:, 3:].reshape(-1, 4, 2), g['corners'], 1e-5, 2e-5, 'GPU G6 _get_ego_dynamics corner points')
    rng = np.random.default_rng(3)                              # and on random states, incl. v_x = 0 (r_bound = miu g / 1e-8)
    ego = np.stack([rng.uniform(0, 9, 5000), rng.normal(0, 1, 5000), rng.normal(0, 1, 5000), rng.uniform(-60, 60, 5000),
                    rng.uniform(-60, 60, 5000), rng.uniform(-400, 400, 5000)], 1).astype(np.float32)
    ego[::50, 0] = 0.0
    par = np.stack([rng.normal(0, 0.1, 5000), rng.normal(0, 0.1, 5000), rng.uniform(0.2, 0.8, 5000), rng.uniform(0.2, 0.8, 5000)], 1).astype(np.float32)
    assert np.array_equal(dev.ego_dynamics(ego, par), host.ego_dynamics(ego, par))


def test_g7_config1_single_env_200_steps_on_gpu():
    """BASELINE configs[0] on the GPU: one env, 8 vehicles, 200 steps, against the reference's trace."""
    g = golden('g7_config1_left')
    modes = [str(m) for m in g['modes']]
    dev = DeviceModel('left', mode='selecting')
    H = g['actions'].shape[0]
    ref = np.array([int(g['ref_index'])], np.int32)
    ego, veh, obs = g['ego'][0:1].copy(), g['veh'][0].copy(), g['obs'][0:1].copy()
    cmode = np.array([[_capi.VMODE_ID[m] for m in modes]], np.uint8)
    for t in range(H):
        act = dev.action_transform(g['actions'][t:t + 1])
        out5, _ = dev.compute_rewards(obs, act)
        ego, params = dev.env_ego_step(ego, act)
        veh = dev.veh_predict(veh.reshape(1, -1)).reshape(-1, 4)
        obs = dev.get_obs(ego, veh[None], cmode, np.zeros(1, np.uint8), ref_idx=ref)
        done = dev.judge_done(ego, params, obs, veh[None], cmode, None, np.zeros(1, np.uint8))
        close(out5[0, 0], g['reward'][t], 1e-5, FIX_ATOL, 'GPU G7 200-step closed loop: reward')
        close(obs[0], g['obs'][t + 1], 1e-5, FIX_ATOL, 'GPU G7 200-step closed loop: obs')
        assert done[0] == g['done_code'][t], 't=%d' % t


from tests._env_step_check import random_scene as _random_scene  # noqa: E402


@pytest.mark.parametrize('task', TASKS)
def test_env_kernels_random_scenes_bit_exact(task):
    B, M = 700, 23
    host, dev = _pair(task, n_veh=VEH_NUM[task])
    ego, cand, cmode, lw, light, act, ref = _random_scene(task, B, M, 31)
    (e_h, p_h), (e_d, p_d) = host.env_ego_step(ego, act), dev.env_ego_step(ego, act)
    assert np.array_equal(e_h, e_d) and np.array_equal(p_h, p_d)
    o_h = host.get_obs(e_h, cand, cmode, light, ref_idx=ref)
    o_d = dev.get_obs(e_h, cand, cmode, light, ref_idx=ref)
    assert np.array_equal(o_h, o_d)
    for lw_ in (lw, None):
        d_h = host.judge_done(e_h, p_h, o_h, cand, cmode, lw_, light)
        d_d = dev.judge_done(e_h, p_h, o_h, cand, cmode, lw_, light)
        assert np.array_equal(d_h, d_d)
    assert len(set(d_h.tolist())) >= 3      # several outcomes occur
    # no candidates at all: every slot takes its fill value (E2E:439-447)
    z_h = host.get_obs(e_h, cand[:, :0], cmode[:, :0], light, ref_idx=ref)
    z_d = dev.get_obs(e_h, cand[:, :0], cmode[:, :0], light, ref_idx=ref)
    assert np.array_equal(z_h, z_d)


@pytest.mark.parametrize('task', TASKS)
def test_get_obs_egos_off_the_map(task):
    """egos that have left the closest-point cell grid (far outside the junction, +-inf, NaN) take the pruned full search
    of the observation kernel: same table index as the oracle's full scan, so the same tracking columns bit for bit"""
    B, M = 300, 9
    host, dev = _pair(task, n_veh=VEH_NUM[task])
    ego, cand, cmode, lw, light, act, ref = _random_scene(task, B, M, 77)
    rng = np.random.default_rng(5)
    ego[:, 3] = rng.uniform(-900, 900, B).astype(np.float32)
    ego[:, 4] = rng.uniform(-900, 900, B).astype(np.float32)
    ego[::7, 3] = rng.uniform(-45, 45, len(ego[::7]))               # a few back on the map, in the same waves
    ego[::7, 4] = rng.uniform(-45, 45, len(ego[::7]))
    ego[5, 3], ego[11, 4], ego[17, 3], ego[23, 4] = np.nan, np.nan, np.inf, -np.inf
    o_h = host.get_obs(ego, cand, cmode, light, ref_idx=ref)
    o_d = dev.get_obs(ego, cand, cmode, light, ref_idx=ref)
    assert np.array_equal(o_h, o_d, equal_nan=True)
    assert np.isfinite(o_h[:, 6]).mean() > 0.9


@pytest.mark.parametrize('task', TASKS)
def test_closest_point_levels_hold_the_reference_argmin_in_every_cell(task):
    """eb_debug_check_grids: the four nested grids the kernels consult instead of scanning the stride-10 table (0.5 m / 4 m / 32 m /
    256 m cells; ranges narrowed by witnesses, medial-axis cells with two ranges or deferred to the next level) — six positions in
    EVERY cell of every level and path (uniform, against the edges, into the corners), mapped to their cell with the kernels' fp32
    expression: the reference's first-minimum argmin over the whole table (DAM:712-714) lies inside the cell's range(s), every time."""
    import ctypes as C
    dev = DeviceModel(task, mode='training')
    n, bad = C.c_int64(), C.c_int64()
    dev.api.debug_check_grids(dev.h, 6, 12345, C.byref(n), C.byref(bad))
    assert n.value > 1_000_000 and bad.value == 0, (n.value, bad.value)


@pytest.mark.parametrize('task', TASKS)
def test_closest_point_on_the_coarse_grid_level(task):
    """Positions from 15 m to 7 km beyond the junction (an ego that finished and drives on): past the 0.5 m corridor grid the kernels
    look the index range up in 8 m cells (out to 400 m around the paths), then in 256 m cells (out to 6.4 km); cells abreast of a long
    straight hold 'long' and take the pruned full search, as everything farther out — the oracle's full scan bit for bit, through the
    one-launch observation (every tile shape), the per-step rollout kernel and the open-loop tape kernel (tables staged in LDS)."""
    B, M = 6000, 6
    host, dev = _pair(task, n_veh=VEH_NUM[task])
    ego, cand, cmode, lw, light, act, ref = _random_scene(task, B, M, 91)
    rng = np.random.default_rng(17)
    r, th = np.where(rng.random(B) < 0.7, rng.uniform(40, 560, B), rng.uniform(560, 7000, B)), rng.uniform(-np.pi, np.pi, B)
    ego[:, 3], ego[:, 4] = (r * np.cos(th)).astype(np.float32), (r * np.sin(th)).astype(np.float32)
    lanes = rng.random(B) < 0.5                                       # half of them straight on along an exit lane, where finished egos go
    side = rng.integers(0, 4, B)
    along, off = np.where(rng.random(B) < 0.7, rng.uniform(30, 520, B), rng.uniform(520, 6800, B)), rng.uniform(-8, 8, B)
    ex = np.where(side == 0, off, np.where(side == 1, off, np.where(side == 2, along, -along)))
    ey = np.where(side == 0, along, np.where(side == 1, -along, np.where(side == 2, off, off)))
    ego[lanes, 3], ego[lanes, 4] = ex[lanes].astype(np.float32), ey[lanes].astype(np.float32)
    o_h = host.get_obs(ego, cand, cmode, light, ref_idx=ref)
    for tile in (0, 1, 2):
        dev.set_tile(tile)
        assert np.array_equal(o_h, dev.get_obs(ego, cand, cmode, light, ref_idx=ref)), tile
    dev.set_tile(-1)
    # many more positions through the one observation kernel: every coarse cell within reach gets a few (the ranges are narrowed by
    # witnesses on the host — eb_capi.hip:build_cell_grid — and a cell whose range missed a position's first minimum would show here)
    Bd = 60000
    cd, cmd = np.tile(cand[:1], (Bd, 1, 1)), np.tile(cmode[:1], (Bd, 1))
    for reach in (470.0, 6900.0):                                     # the 8 m level and the 256 m level (and a rim beyond each)
        egd = np.zeros((Bd, 6), np.float32)
        egd[:, 3], egd[:, 4] = rng.uniform(-reach, reach, Bd).astype(np.float32), rng.uniform(-reach, reach, Bd).astype(np.float32)
        egd[:, 5] = rng.uniform(-180, 180, Bd).astype(np.float32)
        refd = rng.integers(0, int(ref.max()) + 1, Bd).astype(np.int32)
        assert np.array_equal(host.get_obs(egd, cd, cmd, np.zeros(Bd, np.uint8), ref_idx=refd)[:, :9],
                              dev.get_obs(egd, cd, cmd, np.zeros(Bd, np.uint8), ref_idx=refd)[:, :9]), reach
    # beyond every level (> 16 km) and NaN / inf: a few such lanes per wave are searched by the wave together (eight table entries per
    # lane, wave-wide first minimum), a wave full of them lane by lane (the pruned search) — both against the oracle's full scan
    for share in (1.0 / 16.0, 1.0):
        egd = np.zeros((4096, 6), np.float32)
        egd[:, 3], egd[:, 4] = rng.uniform(-60, 10, 4096).astype(np.float32), rng.uniform(-60, 10, 4096).astype(np.float32)
        out = rng.random(4096) < share
        rr, tt = rng.uniform(17000, 90000, 4096), rng.uniform(-np.pi, np.pi, 4096)
        egd[out, 3], egd[out, 4] = (rr * np.cos(tt)).astype(np.float32)[out], (rr * np.sin(tt)).astype(np.float32)[out]
        egd[5::97, 3] = np.nan; egd[7::89, 4] = np.inf; egd[11::83, 3] = -np.inf
        refd = rng.integers(0, int(ref.max()) + 1, 4096).astype(np.int32)
        for tile in (0, 1, 2):
            dev.set_tile(tile)
            assert np.array_equal(host.get_obs(egd, cd[:4096], cmd[:4096], np.zeros(4096, np.uint8), ref_idx=refd)[:, :9],
                                  dev.get_obs(egd, cd[:4096], cmd[:4096], np.zeros(4096, np.uint8), ref_idx=refd)[:, :9], equal_nan=True), (share, tile)
        dev.set_tile(-1)
    # the rollout kernels: rows whose NEXT pose is out there
    nv = VEH_NUM[task]
    inp = make_rollout_inputs(task, B, nv, 3, seed=5)
    obs = np.concatenate([ego, np.zeros((B, 3), np.float32), inp['veh']], 1).astype(np.float32)
    for tile in (-1, 1, 2):
        dev.set_tile(tile)
        a, b = host.rollout_step(obs, inp['actions'][0], ref_idx=ref), dev.rollout_step(obs, inp['actions'][0], ref_idx=ref)
        assert np.array_equal(a[0][:, :9], b[0][:, :9]), tile
    dev.set_tile(-1)
    a, b = host.rollout_tape(obs, inp['actions'], ref_idx=ref), dev.rollout_tape(obs, inp['actions'], ref_idx=ref)
    assert np.array_equal(a[0][:, :9], b[0][:, :9])
    # egos anywhere INSIDE the junction (where nobody drives: between the legs of a turn lie the corridor cells on the path's medial
    # axis, which defer to the 4 m level — or, in the tape kernel, to the pruned search): observation, per-step and tape kernels
    ego[:, 3], ego[:, 4] = rng.uniform(-45, 45, B).astype(np.float32), rng.uniform(-45, 45, B).astype(np.float32)
    ego[:, 0] = rng.uniform(0, 3, B).astype(np.float32)
    assert np.array_equal(host.get_obs(ego, cand, cmode, light, ref_idx=ref), dev.get_obs(ego, cand, cmode, light, ref_idx=ref))
    obs = np.concatenate([ego, np.zeros((B, 3), np.float32), inp['veh']], 1).astype(np.float32)
    a, b = host.rollout_step(obs, inp['actions'][0], ref_idx=ref), dev.rollout_step(obs, inp['actions'][0], ref_idx=ref)
    assert np.array_equal(a[0][:, :9], b[0][:, :9])
    a, b = host.rollout_tape(obs, inp['actions'], ref_idx=ref), dev.rollout_tape(obs, inp['actions'], ref_idx=ref)
    assert np.array_equal(a[0][:, :9], b[0][:, :9])


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('M,NV', [(1, None), (4, None), (33, None), (64, None), (48, 32), (64, 64)])
def test_get_obs_candidate_and_slot_counts(task, M, NV):
    """The observation kernel's LDS-staged form over candidate counts (odd / even row strides, one per env, the
    64-slot maximum) and slot lists with up to 16 slots per mode (deep ranks), plus the fused done code of
    eb_env_step's second half against the two separate calls."""
    B = 257
    nv = VEH_NUM[task] if NV is None else NV
    host, dev = _pair(task, n_veh=nv)
    ego, cand, cmode, lw, light, act, ref = _random_scene(task, B, M, 100 + M)
    cand[:, :, :2] *= 0.5                      # crowd the junction: many in-range candidates per mode
    o_h = host.get_obs(ego, cand, cmode, light, ref_idx=ref)
    o_d = dev.get_obs(ego, cand, cmode, light, ref_idx=ref)
    assert np.array_equal(o_h, o_d)
    empty = host.get_obs(ego, cand[:, :0], cmode[:, :0], light, ref_idx=ref)      # every slot on its fill value
    assert M < 4 or (o_h != empty).any(1).mean() > 0.5                            # real candidates were selected


@pytest.mark.parametrize('task,B,M,NV,nf', __import__('tests._env_step_check', fromlist=['CASES']).CASES)
@pytest.mark.parametrize('tile', [0, 1, 2])
def test_env_step_composite_equals_the_six_calls(task, B, M, NV, nf, tile):
    """eb_env_step == action_transform, compute_rewards, env_ego_step, veh_predict, get_obs, judge_done (+ traffic_respawn
    when a re-entry rule is given) in that order, on both libraries (bit for bit against the oracle's composite too).
    The HIP library runs the composite as ONE launch (csrc/eb_env_step.hip) with 64- / 32- / 16-env tiles (tile 0 / 1 / 2);
    the last case does not fit 64-env tiles and takes the small ones either way: partial tiles, 1..64 candidates,
    non-native slot counts and look-ahead columns go through the same check (tests/_env_step_check.py)."""
    from tests._env_step_check import composite_case
    outs = [composite_case(record_host, task, B, M, NV, nf),
            composite_case(lambda t, **kw: DeviceModel(t, **kw), task, B, M, NV, nf, tile=tile)]
    for a, b in zip(*outs):
        if a.dtype == np.float32 and a.shape == (5, B):
            _check_out5(b, a, 'composite')
        elif a.shape == (16, B):
            bits_equal(b, a, 'reward dictionary')
        else:
            assert np.array_equal(a, b)


def _compare_auto_reset(a, b, B, what):
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None:
            assert y is None
        elif x.dtype == np.float32 and x.shape == (5, B):
            _check_out5(y, x, what)
        elif x.shape == (16, B):
            bits_equal(y, x, '%s: reward dictionary' % what)
        else:
            assert np.array_equal(x, y, equal_nan=True), (what, k)


@pytest.mark.parametrize('task,B,M,NV,nf,vln', [('left', 700, 16, None, 0, False), ('straight', 333, 10, None, 1, False),
                                                 ('right', 130, 20, 7, 0, True), ('left', 260, 64, 16, 0, False),
                                                 ('left', 100, 64, 64, 0, False)])
@pytest.mark.parametrize('tile', [0, 1, 2])
def test_env_step_with_auto_reset(task, B, M, NV, nf, vln, tile):
    """ABI 4 — "step, then reset the envs it has just finished" as ONE launch (env_step_kernel<.., AUTO>): equal to eb_env_step ->
    terminal rows -> eb_env_reset_pool(mask = done != 0) on the HIP library (asserted inside the case), and to the oracle's
    composite bit for bit; every tile shape, a nullable v_light, look-ahead columns, non-native slot counts, 64 candidates."""
    from tests._env_step_check import auto_reset_case
    want = auto_reset_case(record_host, task, B, M, NV=NV, nf=nf, v_light_none=vln)
    got = auto_reset_case(lambda t, **kw: DeviceModel(t, **kw), task, B, M, NV=NV, nf=nf, tile=tile, v_light_none=vln)
    _compare_auto_reset(want, got, B, 'auto reset')


@pytest.mark.parametrize('task,B,M', [('left', 700, 16), ('right', 130, 20), ('straight', 260, 60)])
@pytest.mark.parametrize('tile', [0, 1, 2])
def test_env_step_with_the_episode_step_limit(task, B, M, tile):
    """ABI 5, eb_time_limit in the step's own launch (wave 3 keeps the counts next to the ego-only done predicates): gym's TimeLimit
    around the registered env (README.md:55-59) — asserted against the plain step inside the case, against the oracle's composite
    here; with the reset of the finished (incl. truncated) envs in the same launch; every tile shape."""
    from tests._env_step_check import time_limit_case
    want = time_limit_case(record_host, task, B, M)
    got = time_limit_case(lambda t, **kw: DeviceModel(t, **kw), task, B, M, tile=tile)
    _compare_auto_reset(want[:12], got[:12], B, 'time limit + auto reset')
    assert np.array_equal(want[12], got[12])


def test_parked_ego_is_truncated_at_the_step_limit_on_gpu():
    """201 closed-loop steps of an ego parked on its approach lane: no reference predicate ever fires; code 7 at step 200"""
    from tests._env_step_check import parked_ego_case
    want = parked_ego_case(record_host)
    got = parked_ego_case(lambda t, **kw: DeviceModel(t, **kw))
    assert np.array_equal(want, got)


def test_time_limit_on_the_separate_launch_path():
    """candidates that are not 16-byte aligned: the step's separate launches + the time-limit kernel — the one-launch kernel's bits"""
    import ctypes as C
    import torch
    task, B, M = 'left', 300, 12
    native = VEHICLE_MODE_LIST[task]
    modes = [native[i % len(native)] for i in range(M)]
    ego, cand, _, _, light, _, ref = _random_scene(task, B, M, 23)
    cmode = np.tile(np.array([_capi.VMODE_ID[m] for m in modes], np.uint8), (B, 1))
    rng = np.random.default_rng(4)
    raw = rng.uniform(-1.2, 1.2, (B, 2)).astype(np.float32)
    steps = rng.integers(0, 9, B).astype(np.int32)
    m, tr = DeviceModel(task, mode='training'), DeviceModel(task, n_veh=M, modes=modes)
    obs0 = m.get_obs(ego, cand, cmode, light, ref_idx=ref)
    want = m.env_step(tr, obs0, raw, ego, cand, cmode, ref_idx=ref, v_light=light, time_limit=(steps, 7))
    t, p = torch, lambda x: C.c_void_p(x.data_ptr())
    big = m._in(np.concatenate([np.zeros(1, np.float32), cand.ravel()]))
    c_io = big[1:].view(B, M, 4)                                          # 4 bytes off a 16-byte boundary
    assert c_io.data_ptr() % 16 != 0
    e_io, ob, rw, ri = m._in(ego.copy()), m._in(obs0), m._in(raw), m._in(ref, np.int32)
    cm, vl, es = m._in(cmode, np.uint8), m._in(light, np.uint8), m._in(steps, np.int32)
    par, sc, out5, dd = m._out((B, 4)), m._out((B, 2)), m._out((5, B)), m._out((16, B))
    obs_o, code = m._out(obs0.shape), m._out((B,), np.uint8)
    tl = _capi.EbTimeLimit(es.data_ptr(), 7)
    m.api.env_step(m.h, tr.h, B, p(ob), p(rw), p(ri), 0, p(e_io), p(par), M, p(c_io), p(cm), None, p(vl), None, p(sc), p(out5), p(dd),
                   p(obs_o), p(code), None, None, None, C.byref(tl), m.stream)
    t.cuda.synchronize()
    got = [x.cpu().numpy() for x in (sc, out5, dd, e_io, par, c_io.contiguous(), obs_o, code, es)]
    assert (got[7] == 7).any() and (got[7] == 0).any()
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w), k


@pytest.mark.parametrize('traffic', ['pool', 'flows'])
def test_facade_episode_step_limit(traffic):
    """make('CrossroadEnd2end-v0') = the env inside its registered step limit (README.md:55-59): done_type 'time_limit' and
    info['TimeLimit.truncated'] when nothing else ended the episode, the count kept on the device, restarted by every reset —
    with the reset in the step's launch (pool), composed by the facade (flows), and issued by the caller."""
    from env_build_amd.endtoend import MAX_EPISODE_STEPS, make
    assert MAX_EPISODE_STEPS == 200
    assert make(training_task='left', n_env=4).max_episode_steps == 200
    with pytest.raises(ValueError):
        make('CartPole-v0')
    B, L = 300, 6
    env = make(training_task='left', n_env=B, mode='training', traffic=traffic, auto_reset=True, max_episode_steps=L)
    man = make(training_task='left', n_env=B, mode='training', traffic=traffic, max_episode_steps=L)
    for e in (env, man):
        e.seed(9)
        e.reset()
        e.reset()
    assert (env._episode_step.cpu().numpy() == 0).all()
    count = np.zeros(B, np.int64)
    rng = np.random.default_rng(2)
    n_trunc = 0
    for t in range(3 * L + 2):
        act = rng.uniform(-0.3, 0.3, (B, 2)).astype(np.float32)
        _, _, done, info = env.step(act)
        _, _, done_m, info_m = man.step(act)
        code = env.done_type.numpy()
        count += 1
        trunc = info['TimeLimit.truncated'].numpy() != 0
        assert np.array_equal(trunc, code == 7) and np.array_equal(done.numpy() != 0, code != 0)
        assert np.array_equal(trunc, (count >= L) & ~np.isin(code, [1, 2, 3, 4, 5, 6]))
        count[code != 0] = 0
        assert np.array_equal(env._episode_step.cpu().numpy(), count)
        assert np.array_equal(man.done_type.numpy(), code) and np.array_equal(info_m['TimeLimit.truncated'].numpy() != 0, trunc)
        man.reset(mask=done_m)
        assert np.array_equal(man._episode_step.cpu().numpy(), count)
        n_trunc += int(trunc.sum())
    assert n_trunc > B                                                    # most envs ran into the limit, more than once
    one = make(training_task='left', max_episode_steps=3)                 # the reference-shaped single env
    one.reset()
    for t in range(3):
        _, _, d, info = one.step(np.array([0.0, 0.0], np.float32))
        assert info['TimeLimit.truncated'] is (one.done_type == 'time_limit') and d == int(one.done_type != 'not_done_yet')
        if d:
            break
    assert d == 1 and (one.done_type == 'time_limit') == (t == 2 and info['TimeLimit.truncated'])
    one.reset()
    assert int(one._episode_step.item()) == 0


def test_auto_reset_argument_checks_on_the_gpu():
    from tests._env_step_check import auto_reset_bad_args_case
    auto_reset_bad_args_case(lambda t, **kw: DeviceModel(t, **kw))


def test_auto_reset_on_the_separate_launch_path():
    """Candidates that are not 16-byte aligned: eb_env_step(auto_reset) runs the step's separate launches, the masked row copy
    and eb_env_reset_pool's four launches — the same bits as the one-launch kernel."""
    import ctypes as C
    import torch
    from env_build_amd.endtoend import _lane_entry
    task, B, M = 'left', 400, 12
    native = VEHICLE_MODE_LIST[task]
    modes = [native[i % len(native)] for i in range(M)]
    entry = np.array([list(_lane_entry(m)[:3]) + list(_lane_entry(m)[3]) for m in modes], np.float32)
    ego, cand, _, _, light, _, ref = _random_scene(task, B, M, 17)
    ego[::5, 3] += 9.0                                                   # a fifth of the egos off the road: they finish
    cmode = np.tile(np.array([_capi.VMODE_ID[m] for m in modes], np.uint8), (B, 1))
    rng = np.random.default_rng(6)
    raw = rng.uniform(-1.1, 1.1, (B, 2)).astype(np.float32)
    virtual = (rng.random(B) < 0.5).astype(np.uint8)
    m, tr = DeviceModel(task, mode='training'), DeviceModel(task, n_veh=M, modes=modes)
    obs0 = m.get_obs(ego, cand, cmode, light, ref_idx=ref, virtual=virtual)
    pool = dict(entry=entry, span=60.0, v_max=8.0, seed=4242, counter=17, edge_span=5.0)
    ar = dict(seed=99, counter=5, training=1, pool=pool)
    want = m.env_step(tr, obs0, raw, ego, cand, cmode, ref_idx=ref, v_light=light, virtual=virtual, auto_reset=ar)
    assert 0.05 < (want[7] != 0).mean() < 0.9
    t, dev = torch, m.dev
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    big = t.zeros(B * M * 4 + 1, dtype=t.float32, device=dev)
    c_io = big[1:].view(B, M, 4)                                         # 4-byte aligned only
    c_io.copy_(t.from_numpy(cand))
    e_io, ob, rw, ri = m._in(ego.copy()), m._in(obs0), m._in(raw), m._in(ref, np.int32)
    cm, vl, vf, en = m._in(cmode, np.uint8), m._in(light, np.uint8), m._in(virtual, np.uint8), m._in(entry)
    par, sc, out5, dd = m._out((B, 4)), m._out((B, 2)), m._out((5, B)), m._out((16, B))
    obs_o, code = m._out(obs0.shape), m._out((B,), np.uint8)
    fo = m._in(np.full(obs0.shape, np.nan, np.float32))
    rs = _capi.EbRespawn(en.data_ptr(), 0.0, 60.0, 8.0, 4242, 17, 5.0)
    a = _capi.EbAutoReset(99, 5, 1, ri.data_ptr(), vf.data_ptr(), vl.data_ptr(), rs, fo.data_ptr())
    m.api.env_step(m.h, tr.h, B, p(ob), p(rw), p(ri), 0, p(e_io), p(par), M, p(c_io), p(cm), None, p(vl), p(vf), p(sc), p(out5), p(dd),
                   p(obs_o), p(code), None, C.byref(a), None, None, m.stream)
    t.cuda.synchronize()
    got = [x.cpu().numpy() for x in (sc, out5, dd, e_io, par, c_io.contiguous(), obs_o, code, ri, vf, vl, fo)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w, equal_nan=True), k


@pytest.mark.parametrize('task,K,tile', [('left', 5, -1), ('left', 5, 1), ('straight', 5, 2), ('right', 2, 0), ('left', 1, -1), ('straight', 3, 1)])
def test_env_step_with_the_flow_rule(task, K, tile):
    """ABI 4 — the flow source's step (exits, accelerations, emissions, mode bytes, clock and light) as the last stage of the step's
    own launch: equal to eb_env_step -> eb_traffic_flow_step on the HIP library over a 40-step closed loop (asserted inside the
    case), and to the oracle's composite bit for bit at every step; 12 .. 60 slots, every tile shape that fits."""
    from tests._env_step_check import flow_rule_case
    want = flow_rule_case(record_host, task, B=300, K=K)
    got = flow_rule_case(lambda t, **kw: DeviceModel(t, **kw), task, B=300, K=K, tile=tile)
    for t, (a, b) in enumerate(zip(want, got)):
        _compare_auto_reset(a, b, 300, 'flow rule, step %d' % t)


@pytest.mark.parametrize('task,K,tile', [('left', 5, -1), ('straight', 3, 2), ('right', 5, 1), ('left', 2, 2)])
def test_flow_rule_exit_test_on_records_no_source_would_make(task, K, tile):
    """The exit rule asks for the SIGN of x cos + y sin at a record's new heading.  The 16-env tiles answer it from the sin / cos the
    prediction has just computed whenever that is safe and fall back to the exact expression otherwise: far-out records at any
    heading — tangential ones (the sum within rounding of zero), many-turn headings, box-to-far jumps, NaN / inf fields — come out as
    the two-call composite's and the oracle's, bit for bit (NaN positions equal as NaN)."""
    from tests._env_step_check import flow_rule_case
    want = flow_rule_case(record_host, task, B=300, K=K, steps=3, strict=False, hostile=True)
    got = flow_rule_case(lambda t, **kw: DeviceModel(t, **kw), task, B=300, K=K, tile=tile, steps=3, strict=False, hostile=True)
    for t, (a, b) in enumerate(zip(want, got)):
        _compare_auto_reset(a, b, 300, 'flow rule on hostile records, step %d' % t)


@pytest.mark.parametrize('task,K,tile', [('left', 5, -1), ('left', 5, 1), ('straight', 5, 2), ('right', 2, 0), ('left', 1, -1), ('right', 3, 1)])
def test_env_step_with_the_flow_rule_and_auto_reset(task, K, tile):
    """ABI 5 — the step over the flow source that also resets the envs it finished, ONE launch (the flow source's reset —
    Traffic.init_traffic's role, TRF:151-195 — in the step kernel's tail): equal to eb_env_step(flow) -> final rows -> eb_env_reset ->
    eb_traffic_flow_reset -> eb_get_obs(mask) -> flag swap on the HIP library (asserted inside the case) and to the oracle's composite
    bit for bit at every step of a closed loop in which egos do finish; 12 .. 60 slots, every tile shape that fits."""
    from tests._env_step_check import flow_auto_reset_case
    want = flow_auto_reset_case(record_host, task, B=260, K=K)
    got = flow_auto_reset_case(lambda t, **kw: DeviceModel(t, **kw), task, B=260, K=K, tile=tile)
    for t, (a, b) in enumerate(zip(want, got)):
        _compare_auto_reset(a, b, 260, 'flow rule + auto reset, step %d' % t)


def test_flow_rule_and_auto_reset_on_the_separate_launch_path():
    """candidates that are not 16-byte aligned: eb_env_step(flow + auto_reset) as the step's separate launches, eb_traffic_flow_step and
    the masked reset's launches — the one-launch kernel's bits"""
    import ctypes as C
    import torch
    from env_build_amd.traffic import ACCEL, EXIT_RANGE, FLOWS, LANE_START, ROUTES, VTYPES, approach_lane
    task, B, K = 'left', 200, 2
    M = 12 * K
    slot_modes = [r for r in ROUTES for _ in range(K)]
    lane = np.array([list(approach_lane(x)[0]) + list(approach_lane(x)[1]) for x in slot_modes], np.float32)
    period = (np.array([3600.0 / FLOWS[r][0] for r in ROUTES], np.float32) / 8).astype(np.float32)
    vmax = np.array([VTYPES[FLOWS[x][1]][2] for x in slot_modes], np.float32)
    clen = np.array([VTYPES[FLOWS[x][1]][0] for x in slot_modes], np.float32)
    rng = np.random.default_rng(5)
    inp = make_rollout_inputs(task, B, 8, 1, seed=5)
    ego, ref = inp['ego'].copy(), inp['ref_idx'].copy()
    ego[::4, 3] += 9.0
    m, tr = DeviceModel(task, mode='training'), DeviceModel(task, n_veh=M, modes=slot_modes)
    active = (rng.random((B, M)) < 0.5).astype(np.uint8)
    along = rng.uniform(0, 95, (B, M)).astype(np.float32)
    cand = np.stack([lane[None, :, 0] + along * lane[None, :, 3], lane[None, :, 1] + along * lane[None, :, 4],
                     rng.uniform(0, 9, (B, M)).astype(np.float32), np.broadcast_to(lane[None, :, 2], (B, M))], 2).astype(np.float32)
    mode = np.where(active != 0, np.array([_capi.VMODE_ID[x] for x in slot_modes], np.uint8)[None, :], _capi.VMODE_EMPTY).astype(np.uint8)
    timer = (rng.random((B, 12)) * period).astype(np.float32)
    emitted, sim_step = np.zeros((B, 12), np.int32), rng.integers(0, 600, B).astype(np.int32)
    light, virtual, phase0 = rng.integers(0, 4, B).astype(np.uint8), (rng.random(B) < 0.3).astype(np.uint8), np.full(B, 9, np.uint8)
    raw = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
    obs0 = m.get_obs(ego, cand, mode, light, ref_idx=ref, virtual=virtual)
    flow = dict(per_route=K, lane=lane, period=period, v_max=vmax, dt=0.1, exit_range=EXIT_RANGE, accel=ACCEL, lane_len=LANE_START - 25.0,
                light_cycle=1, seed=99, counter=3, active=active, timer=timer, emitted=emitted, sim_step=sim_step)
    auto = dict(seed=777, counter=4, training=1, flow=dict(cand_len=clen, phase0=phase0, random_phase=0, seed=4242, counter=4))
    want = m.env_step(tr, obs0, raw, ego, cand, mode, ref_idx=ref, v_light=light, virtual=virtual, flow=flow, auto_reset=auto)
    assert (want[7] != 0).sum() > 20
    t, p = torch, lambda x: C.c_void_p(x.data_ptr())
    big = m._in(np.concatenate([np.zeros(1, np.float32), cand.ravel()]))
    c_io = big[1:].view(B, M, 4)
    assert c_io.data_ptr() % 16 != 0
    e_io, ob, rw, ri = m._in(ego.copy()), m._in(obs0), m._in(raw), m._in(ref.copy(), np.int32)
    cm, vl, vf = m._in(mode.copy(), np.uint8), m._in(light.copy(), np.uint8), m._in(virtual.copy(), np.uint8)
    f_act, f_tim, f_emi, f_sim = m._in(active.copy(), np.uint8), m._in(timer.copy()), m._in(emitted.copy(), np.int32), m._in(sim_step.copy(), np.int32)
    f_lane, f_per, f_vm, f_len, f_ph = m._in(lane), m._in(period), m._in(vmax), m._in(clen), m._in(phase0.copy(), np.uint8)
    par, sc, out5, dd = m._out((B, 4)), m._out((B, 2)), m._out((5, B)), m._out((16, B))
    obs_o, code = m._out(obs0.shape), m._out((B,), np.uint8)
    fo = m._in(np.full(obs0.shape, np.nan, np.float32))
    d = lambda x: x.data_ptr()
    fl = _capi.EbFlowRule(K, d(f_act), d(f_tim), d(f_emi), d(f_sim), d(f_lane), d(f_per), d(f_vm), 0.1, EXIT_RANGE, ACCEL, LANE_START - 25.0, 1, 99, 3,
                          d(cm), d(vl))
    ar = _capi.EbAutoReset(777, 4, 1, d(ri), d(vf), d(vl), _capi.EbRespawn(), d(fo), d(f_len), d(f_ph), 0, 4242, 4)
    m.api.env_step(m.h, tr.h, B, p(ob), p(rw), p(ri), 0, p(e_io), p(par), M, p(c_io), p(cm), None, p(vl), p(vf), p(sc), p(out5), p(dd),
                   p(obs_o), p(code), None, C.byref(ar), C.byref(fl), None, m.stream)
    t.cuda.synchronize()
    got = [x.cpu().numpy() for x in (sc, out5, dd, e_io, par, c_io.contiguous(), obs_o, code, ri, vf, vl, fo, f_ph, f_act, f_tim, f_emi, f_sim, cm, vl)]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w, equal_nan=True), k


def test_flow_rule_argument_checks_on_the_gpu():
    from tests._env_step_check import flow_rule_bad_args_case
    flow_rule_bad_args_case(lambda t, **kw: DeviceModel(t, **kw))


@pytest.mark.parametrize('task', TASKS)
@pytest.mark.parametrize('B,tile', [(150, -1), (1000, 0), (1000, 1), (1000, 2)])
def test_masked_observation_pass(task, B, tile):
    """eb_get_obs(row_mask): the observation pass of a masked reset touches the masked rows only (both tile shapes of the
    one-launch machinery; whole tiles without a masked row leave at once) and equals the oracle's."""
    from tests._env_step_check import masked_obs_case

    def make(t, **kw):
        d = DeviceModel(t, **kw)
        d.set_tile(tile)
        return d
    got = masked_obs_case(make, task, B=B)
    want = masked_obs_case(record_host, task, B=B)
    assert np.array_equal(got, want)


def test_env_step_separate_launches_equal_the_one_launch_kernel():
    """A candidate buffer that is not 16-byte aligned (or more than 64 candidates) takes eb_env_step's separate launches
    — same outputs, bit for bit, as the one-launch kernel on the same scene."""
    import ctypes as C
    import torch
    task, B, M = 'left', 333, 12
    native = VEHICLE_MODE_LIST[task]
    modes = [native[i % len(native)] for i in range(M)]
    ego, cand, _, _, light, _, ref = _random_scene(task, B, M, 91)
    cmode = np.tile(np.array([_capi.VMODE_ID[m] for m in modes], np.uint8), (B, 1))
    rng = np.random.default_rng(6)
    raw = rng.uniform(-1.1, 1.1, (B, 2)).astype(np.float32)
    cand[:, :3, 0] = 70.0                                                # three per env have left the map
    entry = rng.uniform(-50, 50, (M, 5)).astype(np.float32)
    m, tr = DeviceModel(task, mode='training'), DeviceModel(task, n_veh=M, modes=modes)
    obs0 = m.get_obs(ego, cand, cmode, light, ref_idx=ref)
    rule = dict(entry=entry, limit=65.0, span=60.0, v_max=8.0, seed=77, counter=3)
    want = m.env_step(tr, obs0, raw, ego, cand, cmode, ref_idx=ref, v_light=light, respawn=rule)
    # the same call with the candidates one float into a larger buffer: 4-byte aligned only
    t, dev = torch, m.dev
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    big = t.zeros(B * M * 4 + 1, dtype=t.float32, device=dev)
    c_io = big[1:].view(B, M, 4)
    c_io.copy_(t.from_numpy(cand))
    assert c_io.data_ptr() % 16 != 0
    e_io, ob, rw, ri = m._in(ego.copy()), m._in(obs0), m._in(raw), m._in(ref, np.int32)
    cm, vl, en = m._in(cmode, np.uint8), m._in(light, np.uint8), m._in(entry)
    par, sc, out5, dd = m._out((B, 4)), m._out((B, 2)), m._out((5, B)), m._out((16, B))
    obs_o, code = m._out(obs0.shape), m._out((B,), np.uint8)
    rs = _capi.EbRespawn(en.data_ptr(), 65.0, 60.0, 8.0, 77, 3)
    m.api.env_step(m.h, tr.h, B, p(ob), p(rw), p(ri), 0, p(e_io), p(par), M, p(c_io), p(cm), None, p(vl), None, p(sc), p(out5), p(dd),
                   p(obs_o), p(code), C.byref(rs), None, None, None, m.stream)
    t.cuda.synchronize()
    got = [x.cpu().numpy() for x in (sc, out5, dd, e_io, par, c_io.contiguous(), obs_o, code)]
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g).reshape(np.asarray(w).shape), w), k


@pytest.mark.parametrize('task,n_env', [('left', 1), ('straight', 1), ('right', 64), ('left', 300)])
def test_crossroad_env_facade_matches_oracle_composition(task, n_env):
    """CrossroadEnd2end.step / reset (the reference's Gym surface) against the same composition made of oracle
    calls on the env's own traffic state: obs, reward and done code identical at every step."""
    from env_build_amd.endtoend import CrossroadEnd2end
    env = CrossroadEnd2end(task, n_env=n_env, mode='training')
    env.seed(3)
    obs = env.reset()
    host = HostModel(oracle_lib(), task, mode='training')
    traffic = HostModel(oracle_lib(), task, n_veh=env.n_cand, modes=env.cand_modes)
    D = 9 + 4 * VEH_NUM[task]
    assert (obs.shape == (D,) and obs.dtype == np.float32) if n_env == 1 else obs.shape == (n_env, D)
    rng = np.random.default_rng(0)
    cmode = env._cand_mode.cpu().numpy()
    for t in range(12):
        ego0, cand0 = env._ego.cpu().numpy(), env._cand.cpu().numpy()
        obs0, ref = env._obs.cpu().numpy(), env._ref_idx.cpu().numpy()
        if n_env == 1:
            ref = np.array([env.ref_path.ref_index], np.int32)
        v_light, virtual = env._v_light.cpu().numpy(), env._virtual.cpu().numpy()
        action = rng.uniform(-1, 1, (n_env, 2)).astype(np.float32)
        obs, reward, done, info = env.step(action[0] if n_env == 1 else action)
        act = host.action_transform(action)
        o5, d16 = host.compute_rewards(obs0, act)
        ego1, par1 = host.env_ego_step(ego0, act)
        cand1 = traffic.veh_predict(cand0.reshape(n_env, -1)).reshape(n_env, -1, 4)
        gone = (np.abs(cand1[:, :, 0]) > 65) | (np.abs(cand1[:, :, 1]) > 65)
        cand_env = env._cand.cpu().numpy()
        assert np.array_equal(cand_env[~gone], cand1[~gone])              # re-entered vehicles are the env's own business
        obs1 = host.get_obs(ego1, cand1, cmode, v_light, ref_idx=ref, virtual=virtual)   # the step observes the pool before re-entry
        done1 = host.judge_done(ego1, par1, obs1, cand1, cmode, None, v_light)
        if n_env == 1:
            assert isinstance(done, int) and np.asarray(reward).shape == () and 'reward_info' in info
            assert np.array_equal(obs, obs1[0]) and reward == o5[0, 0] and done == int(done1[0] != 0)
            assert env.done_type == _capi.DONE_NAMES[int(done1[0])]
            assert set(info['reward_info']) >= {'punish_steer', 'veh2road4real', 'final_rew'}
            assert len(env.all_vehicles) == env.n_cand and abs(env.ego_dynamics['x'] - ego1[0, 3]) < 1e-6
        else:
            assert np.array_equal(obs.numpy(), obs1) and np.array_equal(reward.numpy(), o5[0])
            assert np.array_equal(env.done_code.cpu().numpy(), done1)


@pytest.mark.parametrize('copy_outputs', [True, False])
def test_facade_auto_reset_equals_step_then_masked_reset(copy_outputs):
    """CrossroadEnd2end(auto_reset=True).step == step() followed by reset(mask=done) of an env with the same seed, step for step:
    observation, reward, done, state; info['final_observation'] holds the terminal rows."""
    from env_build_amd.endtoend import CrossroadEnd2end
    B, task = 1500, 'left'
    a = CrossroadEnd2end(task, n_env=B, mode='training', auto_reset=True, copy_outputs=copy_outputs)
    b = CrossroadEnd2end(task, n_env=B, mode='training', copy_outputs=copy_outputs)
    for env in (a, b):
        env.seed(5)
        env.reset()          # (a reset observation is built with the flags of the episode before, E2E:116-126: the second
        env.reset()          # reset after seed() no longer depends on what the constructor's own warm-up step drew)
    assert np.array_equal(a.obs.numpy(), b.obs.numpy())
    rng = np.random.default_rng(1)
    finished = 0
    for t in range(40):
        act = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, _ = b.step(act)
        fin = db.numpy() != 0
        term = ob.numpy().copy()
        ob = b.reset(mask=db)
        assert np.array_equal(da.numpy(), fin.astype(np.uint8)) and np.array_equal(ra.numpy(), rb.numpy())
        assert np.array_equal(oa.numpy(), ob.numpy()), t
        assert np.array_equal(ia['final_observation'].numpy()[fin], term[fin])
        for k in ('_ego', '_params', '_cand', '_ref_idx', '_virtual', '_v_light'):
            assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), (t, k)
        finished += int(fin.sum())
    assert finished > 20                                                  # episodes did end (and restart) on the way
    with pytest.raises(ValueError):
        CrossroadEnd2end(task, n_env=1, auto_reset=True)


@pytest.mark.parametrize('copy_outputs', [True, False])
def test_facade_auto_reset_over_the_flow_source(copy_outputs):
    """auto_reset over the flow source (composed by the facade: the step's launch, then the masked reset's) == step() followed by
    reset(mask=done) of an env with the same seed; and a masked reset never writes into the observation the last step handed out."""
    from env_build_amd.endtoend import CrossroadEnd2end
    B, task = 600, 'left'
    a = CrossroadEnd2end(task, n_env=B, mode='training', traffic='flows', auto_reset=True, copy_outputs=copy_outputs)
    b = CrossroadEnd2end(task, n_env=B, mode='training', traffic='flows', copy_outputs=copy_outputs)
    for env in (a, b):
        env.seed(5)
        env.reset()
        env.reset()
    assert np.array_equal(a.obs.numpy(), b.obs.numpy())
    rng = np.random.default_rng(1)
    finished = 0
    for t in range(30):
        act = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, _ = b.step(act)
        fin = db.numpy() != 0
        term = ob.numpy().copy()
        ob2 = b.reset(mask=db)
        assert np.array_equal(ob.numpy(), term), 'reset(mask) wrote into the observation the step handed out'
        assert np.array_equal(da.numpy(), fin.astype(np.uint8)) and np.array_equal(ra.numpy(), rb.numpy())
        assert np.array_equal(oa.numpy(), ob2.numpy()), t
        assert np.array_equal(ia['final_observation'].numpy()[fin], term[fin])
        assert np.array_equal(a.done_type.numpy() != 0, fin)                   # done_type stays the step's
        assert np.array_equal(a.done_code.cpu().numpy() != 0, fin)             # ... and so does the public done_code array
        for k in ('_ego', '_params', '_cand_mode', '_ref_idx', '_virtual', '_v_light'):
            assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()), (t, k)
        on = a._cand_mode.cpu().numpy() != 255          # (a vacant slot keeps whatever record it held last: the constructors' warm-up
        assert np.array_equal(a._cand.cpu().numpy()[on], b._cand.cpu().numpy()[on]), t     # steps drew different actions)
        for k in ('active', 'timer', 'emitted', 'sim_step'):
            assert np.array_equal(getattr(a._flows, k).cpu().numpy(), getattr(b._flows, k).cpu().numpy()), (t, k)
        finished += int(fin.sum())
    assert finished > 5


def test_facade_ref_index_is_a_snapshot_made_on_demand():
    """copy_outputs=True: info['ref_index'] is handed out without a copy and gets one when it is read, or right before a reset /
    an auto-reset step rewrites the path indices in place — a value read late still holds its own step's indices."""
    from env_build_amd.endtoend import CrossroadEnd2end
    B = 500
    rng = np.random.default_rng(4)
    for auto in (False, True):
        env = CrossroadEnd2end('left', n_env=B, mode='training', auto_reset=auto)
        env.seed(3)
        env.reset()
        changed = 0
        for t in range(40):
            act = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
            o, r, d, info = env.step(act)
            now = env._ref_idx.cpu().numpy().copy()          # the indices as this step left them
            kept = info['ref_index']                         # not read yet
            if auto:
                env.step(act)                                # the next step rewrites them in place (finished envs draw a new path)
            else:
                env.reset(mask=d)
            assert np.array_equal(kept.numpy(), now), (auto, t)
            changed += int((env._ref_idx.cpu().numpy() != now).sum())
        assert changed > 0


def test_facade_outputs_are_arrays_of_their_own_by_default():
    """what step() hands out can be kept (a rollout list, a replay buffer) — three steps later every stored value still
    holds its own step, `done` and reward_info included when they are first read late; copy_outputs=False is the opt-in
    two-set scheme whose values live until the step after next."""
    from env_build_amd.endtoend import CrossroadEnd2end
    B = 300
    env = CrossroadEnd2end('left', n_env=B, mode='training', auto_reset=True)
    ref = CrossroadEnd2end('left', n_env=B, mode='training', auto_reset=True)
    for e in (env, ref):
        e.seed(9)
        e.reset()
        e.reset()
    rng = np.random.default_rng(2)
    kept, want = [], []
    for t in range(5):
        act = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
        kept.append(env.step(act))                                        # nothing read yet
        o, r, d, info = ref.step(act)
        want.append((o.numpy().copy(), r.numpy().copy(), d.numpy().copy(), info['reward_info']['punish_steer'].numpy().copy(),
                     info['ref_index'].numpy().copy(), info['final_observation'].numpy().copy()))
    for (o, r, d, info), w in zip(kept, want):
        fin = w[2] != 0
        assert np.array_equal(o.numpy(), w[0]) and np.array_equal(r.numpy(), w[1]) and np.array_equal(d.numpy(), w[2])
        assert np.array_equal(info['reward_info'].get('punish_steer').numpy(), w[3])      # computed now, from that step's inputs
        assert np.array_equal(info['ref_index'].numpy(), w[4])
        assert np.array_equal(info['final_observation'].numpy()[fin], w[5][fin])
    # the dict behaves like the dict it stands for
    ri = kept[-1][3]['reward_info']
    assert ri.get('no_such_term') is None and set(ri.copy()) == set(ri.keys()) and len(ri.copy()) == 17
    import pickle
    assert set(pickle.loads(pickle.dumps({k: v.numpy() for k, v in ri.items()}))) == set(ri)
    assert env._want_d16                                                  # from now on the kernel writes the 16 terms itself
    o, r, d, info = env.step(np.zeros((B, 2), np.float32))
    o2, r2, d2, info2 = ref.step(np.zeros((B, 2), np.float32))
    assert np.array_equal(info['reward_info']['veh2road4real'].numpy(), info2['reward_info']['veh2road4real'].numpy())
    st = env.init_state
    assert st.get('ego') is not None and st.get('nothing') is None and list(st.copy()) == ['ego']


# ---- fp16 state storage (BASELINE configs[4]) -------------------------------------------------------------
@pytest.mark.parametrize('tile', [-1, 0, 1, 2])
@pytest.mark.parametrize('task,N,nf', [('left', 64, 0), ('straight', 9, 0), ('right', 64, 2), ('left', 32, 0)])
def test_fp16_storage_bit_exact_against_oracle(task, N, nf, tile):
    """eb_rollout_step_f16: binary16 rows in and out, fp32 arithmetic and fp32 rewards — every half and every
    fp32 output identical to the oracle's widen / fp32 step / round-to-nearest-even, over a closed loop."""
    B, H = 555, 10
    host, dev = _pair(task, n_veh=N, n_future=nf)
    dev.set_tile(tile)
    inp = make_rollout_inputs(task, B, N, H, seed=40 + N, n_future=nf)
    obs_h = obs_d = _initial_obs(host, inp).astype(np.float16).view(np.uint16)
    for t in range(H):
        obs_h, o5_h, sc_h = host.rollout_step_f16(obs_h, inp['actions'][t], inp['ref_idx'])
        obs_d, o5_d, sc_d = dev.rollout_step_f16(obs_d, inp['actions'][t], inp['ref_idx'])
        assert np.array_equal(obs_d, obs_h), 'step %d: %d halves differ' % (t, int((obs_d != obs_h).sum()))
        assert np.array_equal(sc_d, sc_h)
        _check_out5(o5_d, o5_h, 'step %d' % t)
    a, a5 = dev.rollout_tape_f16(obs_d, inp['actions'][:3], inp['ref_idx'])
    b, b5 = host.rollout_tape_f16(obs_h, inp['actions'][:3], inp['ref_idx'])
    assert np.array_equal(a, b)
    bits_equal(a5, b5, 'out5 of every step')


@pytest.mark.parametrize('task', TASKS)
def test_g8_fp16_fixture_on_gpu(task):
    g = golden('g8_fp16_rollout_%s_N64' % task)
    dev = DeviceModel(task, n_veh=64, modes=[str(m) for m in g['modes']])
    for t in range(g['actions'].shape[0]):
        out, o5, _ = dev.rollout_step_f16(g['obs_in'][t], g['actions'][t], g['ref_idx'])
        close(o5, g['out5'][t], 1e-5, FIX_ATOL, 'GPU G8 fp16 state: out5')
        k = lambda u: np.where(u.astype(np.int32) & 0x8000, -(u.astype(np.int32) & 0x7FFF), u.astype(np.int32) & 0x7FFF)
        assert np.abs(k(out) - k(g['obs_out'][t])).max() <= 1, 't=%d' % t


def test_fp16_storage_headline_size_properties():
    """configs[4] at full size (65 536 envs x 64 vehicles, 34.7 MB of halves): sampled rows against the oracle,
    whole-batch invariants."""
    task, B, N = 'left', 65536, 64
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, 2, seed=2)
    rows = np.unique(np.concatenate([np.arange(0, 70), np.arange(B - 70, B), np.random.default_rng(4).integers(0, B, 400)]))
    ego, ref = inp['ego'], inp['ref_idx']
    trk = host.tracking_error(ego[rows, 3], ego[rows, 4], ego[rows, 5], ego[rows, 0], 0, ref_idx=ref[rows])
    obs = assemble_obs(ego, np.zeros((B, 3), np.float32), inp['veh'])
    obs[rows, 6:9] = trk
    obs_d = obs.astype(np.float16).view(np.uint16)
    obs_h = obs_d[rows].copy()
    for t in range(2):
        prev = obs_d
        obs_d, o5_d, _ = dev.rollout_step_f16(obs_d, inp['actions'][t], ref)
        obs_h, o5_h, _ = host.rollout_step_f16(obs_h, inp['actions'][t][rows], ref[rows])
        assert np.array_equal(obs_d[rows], obs_h)
        _check_out5(o5_d[:, rows], o5_h, 'step %d' % t)
        v_in, v_out = prev[:, 9:].reshape(B, N, 4), obs_d[:, 9:].reshape(B, N, 4)
        assert np.array_equal(v_in[:, :, 2], v_out[:, :, 2])                  # speeds carried over bit for bit
        assert np.isfinite(obs_d.view(np.float16).astype(np.float32)).all() and np.isfinite(o5_d).all()


def test_fp16_storage_headline_size_every_row():
    """configs[4] in full — 65 536 envs x 64 vehicles, binary16 state, 25 closed-loop steps, EVERY row against the oracle's tape."""
    task, B, N, H = 'left', 65536, 64, 25
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=8)
    obs0 = _initial_obs(host, inp).astype(np.float16).view(np.uint16)
    out_h, o5_h = host.rollout_tape_f16(obs0, inp['actions'], inp['ref_idx'])
    obs_d = obs0
    for t in range(H):
        obs_d, o5_d, _ = dev.rollout_step_f16(obs_d, inp['actions'][t], inp['ref_idx'])
        _check_out5(o5_d, o5_h[t], 'step %d' % t)
    assert np.array_equal(obs_d, out_h)


def test_environment_model_fp16_state_facade():
    from env_build_amd.dynamics_and_models import EnvironmentModel
    task, B, N = 'left', 200, 64
    host = HostModel(oracle_lib(), task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, 3, seed=6)
    obs16 = _initial_obs(host, inp).astype(np.float16)
    m = EnvironmentModel(task, n_veh=N, state_dtype='float16')
    m.reset(obs16, inp['ref_idx'])
    o_h = obs16.view(np.uint16)
    for t in range(3):
        obses, rewards, p_train, p_real, v2v, v2r = m.rollout_out(inp['actions'][t])
        o_h, o5_h, _ = host.rollout_step_f16(o_h, inp['actions'][t], inp['ref_idx'])
        assert obses.dtype == __import__('torch').float16 and rewards.dtype == __import__('torch').float32
        assert np.array_equal(obses.numpy().view(np.uint16), o_h)
        assert np.array_equal(rewards.numpy(), o5_h[0])


@pytest.mark.parametrize('mode', ['training', 'selecting'])
def test_environment_model_rollout_out_output_sets(mode):
    """EnvironmentModel.rollout_out (DAM:118-126) through the drop-in class: copy_outputs=True hands out arrays of its own every
    call (a list of them keeps every step's values), copy_outputs=False the same values from two sets used in turn — valid until
    the call after next; the 6-tuple, `.obses` and `.actions` (the scaled actions, DAM:120) are the oracle's."""
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    task, B, N, H = 'left', 300, 8, 6
    host = record_host(task, n_veh=N, mode=mode)
    inp = make_rollout_inputs(task, B, N, H, seed=8)
    ref = inp['ref_idx'] if mode == 'training' else None
    obs0 = _initial_obs(HostModel(oracle_lib(), task, n_veh=N), inp)
    a, b = EnvironmentModel(task, mode=mode), EnvironmentModel(task, mode=mode, copy_outputs=False)
    for m in (a, b):
        if mode == 'training':
            m.reset(obs0, ref)
        else:
            m.add_traj(obs0, 1)
    kept_a, kept_b, o_h = [], [], obs0
    for t in range(H):
        ra, rb = a.rollout_out(inp['actions'][t]), b.rollout_out(torch.from_numpy(inp['actions'][t]).cuda())
        o_h, o5_h, sc_h = host.rollout_step(o_h, inp['actions'][t], ref, path_id=1)
        for r, m in ((ra, a), (rb, b)):
            assert len(r) == 6 and r[0] is m.obses
            assert np.array_equal(r[0].numpy(), o_h) and np.array_equal(m.actions.numpy(), sc_h)
            _check_out5(np.stack([x.numpy() for x in r[1:]]), o5_h, 'facade step %d' % t)
        assert (ra[3] + 1.0).numpy().shape == (B,) and float(ra[1][0]) == ra[1].numpy()[0]      # what hier_decision.py:96 does with them
        kept_a.append(ra); kept_b.append((rb, [x.numpy().copy() for x in rb]))
    # arrays of their own: every step's values are still there
    o_h = obs0
    for t in range(H):
        o_h, o5_h, _ = host.rollout_step(o_h, inp['actions'][t], ref, path_id=1)
        assert np.array_equal(kept_a[t][0].numpy(), o_h)
    assert len({r[0].data_ptr() for r in kept_a}) == H
    # two sets in turn: the last two calls' values are intact, older ones have been overwritten by later steps
    assert len({r[0].data_ptr() for r, _ in kept_b}) == 2
    for t in (H - 2, H - 1):
        for x, c in zip(*kept_b[t]):
            assert np.array_equal(x.numpy(), c)
    assert not np.array_equal(kept_b[0][0][0].numpy(), kept_b[0][1][0])


# ---- open-loop tape kernel (eb_rollout_tape: H steps in one launch, state in registers) -----------------------
@pytest.mark.parametrize('tile', [-1, 0, 1, 2])
@pytest.mark.parametrize('task,N,nf,H', [('left', 32, 0, 25), ('straight', 9, 2, 7), ('right', 64, 0, 3), ('left', 16, 0, 1),
                                         ('right', 5, 1, 12)])
def test_tape_kernel_equals_stepwise_launches_and_oracle(task, N, nf, H, tile):
    """One launch over the whole tape == H per-step launches (bit for bit, every output) == the oracle."""
    B = 700
    host, dev = _pair(task, n_veh=N, n_future=nf)
    dev.set_tile(tile)
    inp = make_rollout_inputs(task, B, N, H, seed=60 + N + H, n_future=nf)
    inp['ref_idx'][::13] = 7          # rows without a path
    obs0 = _initial_obs(host, inp)
    out_f, o5_f = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    dev.set_tape_stepwise(True)
    out_s, o5_s = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    dev.set_tape_stepwise(False)
    out_h, o5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(out_f, out_s) and np.array_equal(o5_f, o5_s)
    assert np.array_equal(out_f, out_h)
    for t in range(H):
        _check_out5(o5_f[t], o5_h[t], 'step %d' % t)


@pytest.mark.parametrize('tile', [0, 2])
def test_tape_kernel_crowded_remote_and_special_values(tile):
    """the scenes of test_crowded_and_remote_scenes through the tape kernel: queue drains inside the step loop,
    egos outside the cell grid, stopped / denormal / -0 / non-finite records carried in registers for 6 steps"""
    task, B, N, H = 'left', 300, 32, 6
    host, dev = _pair(task, n_veh=N)
    dev.set_tile(tile)
    inp = make_rollout_inputs(task, B, N, H, seed=78)
    rng = np.random.default_rng(6)
    veh, ego = inp['veh'].reshape(B, N, 4).copy(), inp['ego'].copy()
    veh[:100, :, 0] = ego[:100, None, 3] + rng.uniform(-4, 4, (100, N))
    veh[:100, :, 1] = ego[:100, None, 4] + rng.uniform(-4, 4, (100, N))
    veh[:100, :, 2] = rng.uniform(0, 1.0, (100, N))                      # slow: they stay crowded
    ego[100:150, 3] = rng.uniform(-400, 400, 50); ego[100:150, 4] = rng.uniform(-400, 400, 50)
    veh[160:200, :, 2] = 0.0
    veh[200:220, :, 3] = 0.0
    veh[220:240, :, 3] = np.float32(1e-38)
    veh[240:260, :, 2] = np.float32(3e-39)
    veh[260:280, :, 0:2] = rng.uniform(-20, 20, (20, N, 2)); veh[260:280, :, 2] = 0.0; veh[260:280, :, 3] = -0.0
    veh[290:294, :, 2] = np.inf
    veh[294:297, :, 3] = -np.inf
    veh[297:300, :, 3] = np.float32(2e38)
    inp['ego'], inp['veh'] = ego, veh.reshape(B, 4 * N)
    obs0 = _initial_obs(host, inp)
    out_f, o5_f = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    out_h, o5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    nan_h = np.isnan(out_h)
    assert np.array_equal(nan_h, np.isnan(out_f))
    assert np.array_equal(out_f.view(np.uint32)[~nan_h], out_h.view(np.uint32)[~nan_h])
    for t in range(H):
        ok = ~np.isnan(o5_h[t]).any(0)
        assert np.array_equal(ok, ~np.isnan(o5_f[t]).any(0))
        _check_out5(o5_f[t][:, ok], o5_h[t][:, ok], 'step %d' % t)
    assert (o5_f[:, 1, :100] > 0).all()


@pytest.mark.parametrize('N', [64, 9])
def test_tape_kernel_fp16_storage(N):
    """fp16 storage through the tape kernel: the state is re-rounded to binary16 after every step, as H stores would"""
    task, B, H = 'straight', 400, 9
    host, dev = _pair(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, H, seed=90 + N)
    obs16 = _initial_obs(host, inp).astype(np.float16).view(np.uint16)
    a, a5 = dev.rollout_tape_f16(obs16, inp['actions'], inp['ref_idx'])
    b, b5 = host.rollout_tape_f16(obs16, inp['actions'], inp['ref_idx'])
    assert np.array_equal(a, b)
    for t in range(H):
        _check_out5(a5[t], b5[t], 'step %d' % t)


# ---- odd shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('task,B,N,nf', [('left', 1, 8, 0), ('right', 2, 1, 0), ('straight', 63, 2, 8), ('left', 65, 33, 0),
                                         ('right', 4097, 7, 1), ('straight', 130, 64, 0)])
def test_odd_batch_and_slot_counts(task, B, N, nf):
    """single env, one slot, slot counts that do not divide a wave, batches one past a tile: step and tape"""
    host, dev = _pair(task, n_veh=N, n_future=nf)
    inp = make_rollout_inputs(task, B, N, 4, seed=B + N, n_future=nf)
    obs0 = _initial_obs(host, inp)
    o_h, o5_h, _ = host.rollout_step(obs0, inp['actions'][0], inp['ref_idx'])
    o_d, o5_d, _ = dev.rollout_step(obs0, inp['actions'][0], inp['ref_idx'])
    assert np.array_equal(o_d, o_h)
    _check_out5(o5_d, o5_h, 'step')
    t_h, t5_h = host.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    t_d, t5_d = dev.rollout_tape(obs0, inp['actions'], inp['ref_idx'])
    assert np.array_equal(t_d, t_h)
    bits_equal(t5_d, t5_h, 'out5 of every step')


def test_sharded_batch_size_262144_rows_are_independent():
    """BASELINE configs[3] is 262 144 envs split over 8 GPUs; on one GPU the same batch in one launch must give, row
    for row, what eight 32 768-env shards give (no cross-row state anywhere on the path)."""
    task, B, N = 'left', 262144, 32
    dev = DeviceModel(task, n_veh=N)
    inp = make_rollout_inputs(task, B, N, 1, seed=12)
    obs0 = assemble_obs(inp['ego'], np.zeros((B, 3), np.float32), inp['veh'])
    whole, whole5, _ = dev.rollout_step(obs0, inp['actions'][0], inp['ref_idx'])
    from env_build_amd.sharding import shard_range
    for r in (0, 3, 7):
        lo, hi = shard_range(B, r, 8)
        part, part5, _ = dev.rollout_step(obs0[lo:hi], inp['actions'][0][lo:hi], inp['ref_idx'][lo:hi])
        assert np.array_equal(part, whole[lo:hi]) and np.array_equal(part5, whole5[:, lo:hi])


def test_batched_safety_shield_matches_per_row_reference_logic():
    """env_build_amd.shield.is_safe (hier_decision.py:89-97 for a whole batch): the same verdict and penalty as
    stepping the oracle with the same closed-loop policy"""
    import torch
    from env_build_amd.dynamics_and_models import DevArray, EnvironmentModel
    from env_build_amd.shield import is_safe, safe_shield
    task, B, N = 'left', 600, 8
    host = HostModel(oracle_lib(), task, n_veh=N, mode='selecting')
    inp = make_rollout_inputs(task, B, N, 1, seed=15)
    inp['ref_idx'][:] = 1
    obs0 = _initial_obs(host, inp)

    def policy(obs):               # a fixed linear feedback on the tracking errors, as a stand-in for run_batch
        o = obs.torch() if isinstance(obs, DevArray) else torch.as_tensor(obs)
        return torch.stack([(-0.05 * o[:, 6] - 0.01 * o[:, 7]).clamp(-1, 1), (-0.1 * o[:, 8]).clamp(-1, 1)], 1).contiguous()

    model = EnvironmentModel(task, mode='selecting')
    safe, punish = is_safe(model, policy, obs0, path_index=1, steps=5)
    o, acc = obs0, np.zeros(B, np.float32)
    for _ in range(5):
        a = policy(torch.from_numpy(o)).numpy()
        o, o5, _ = host.rollout_step(o, a, None, 1)
        acc = acc + o5[3]
    np.testing.assert_allclose(punish.numpy(), acc, rtol=1e-5, atol=1e-6)
    assert np.array_equal(safe.numpy(), ~(acc > 0)) and 0 < safe.numpy().sum() < B
    act, started = safe_shield(model, policy, obs0, path_index=1)
    assert np.array_equal(started.numpy(), ~safe.numpy())
    assert np.array_equal(act.numpy()[started.numpy()], np.tile(np.float32([0., -1.]), (int(started.numpy().sum()), 1)))


def test_env_step_and_masked_reset_at_the_bench_size_equal_the_oracle():
    """65 536 envs x 16 candidates — the size `bench.py`'s env_step entry times (1 024 blocks of 64-env tiles, all resident at
    once): every row of the one-launch step and of the one-launch masked reset against the oracle's composites."""
    from tests._env_step_check import composite_case, reset_pool_case
    task, B, M = 'left', 65536, 16
    on_cpu, on_gpu = (record_host), (lambda t, **kw: DeviceModel(t, **kw))
    for a, b in zip(composite_case(on_cpu, task, B, M, None, 0), composite_case(on_gpu, task, B, M, None, 0)):
        if a.dtype == np.float32 and a.shape == (5, B):
            _check_out5(b, a, 'composite 65536')
        elif a.shape == (16, B):
            bits_equal(b, a, 'reward dictionary')
        else:
            assert np.array_equal(a, b)
    for a, b in zip(reset_pool_case(on_cpu, task, B=B, M=M, seed=77), reset_pool_case(on_gpu, task, B=B, M=M, seed=77)):
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), k
    # the step with the reset of the envs it finishes in the same launch (ABI 4), every row
    from tests._env_step_check import auto_reset_case
    _compare_auto_reset(auto_reset_case(on_cpu, task, B, M), auto_reset_case(on_gpu, task, B, M), B, 'auto reset 65536')
