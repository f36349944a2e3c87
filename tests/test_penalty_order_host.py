"""CPU: the oracle's two penalty-sum orders (eb_oracle_set_penalty_order) against tests/_penalty.resum over the terms the oracle
exports (eb_oracle_penalty_terms) — bit for bit, on the scenes the GPU suite runs (tests/test_gpu_penalty_order.py) and on
make_rollout_inputs scenes.  Order 0 (the reference's, the default) is what the fixtures pin; order 1 (by record) is what every HIP
kernel computes, so that the GPU tests can ask for equality instead of PEN_RTOL.
"""
import glob
import os

import numpy as np
import pytest

from env_build_amd.endtoend_env_utils import VEH_NUM
from env_build_amd.synthetic import make_rollout_inputs
from tests import _golden_checks as CK
from tests import _penalty as P
from tests._helpers import GOLDEN, PARITY_LOG, HostModel, close, golden, initial_obs

TASKS = ('left', 'straight', 'right')
SIZES = ('native', 16, 64)
SEED = 20
ORDERS = ('reference', 'record')
_cache = {}


def _case(oracle, task, n_veh):
    """the scenes of (task, n_veh) with their terms and the oracle's out5 / dict in both orders — computed once"""
    N = VEH_NUM[task] if n_veh == 'native' else n_veh
    key = (task, N)
    if key not in _cache:
        sc = P.scenes(task, N, SEED)
        host = HostModel(oracle, task, n_veh=N)
        c = dict(sc, N=N, terms=host.penalty_terms(sc['obs']))
        for order in ORDERS:
            host.set_penalty_order(order)
            c[order] = host.compute_rewards(sc['obs'], sc['actions'][0])
        _cache[key] = c
    return _cache[key]


def _same(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan], want[~nan]), what


def _held_to_resum(host, obs, actions, what):
    terms = host.penalty_terms(obs)
    for order in ORDERS:
        host.set_penalty_order(order)
        out5, d16 = host.compute_rewards(obs, actions)
        w5, w16 = P.expected_out5_rows(*terms, order=order)
        _same(out5[1:], w5, '%s: out5, %s order' % (what, order))
        _same(d16[12:], w16, '%s: dict rows 12-15, %s order' % (what, order))
    return terms


@pytest.mark.parametrize('n_veh', SIZES)
@pytest.mark.parametrize('task', TASKS)
def test_oracle_orders_equal_resum_on_scenes(oracle, task, n_veh):
    c = _case(oracle, task, n_veh)
    assert len(c['obs']) <= P.MAX_ROWS
    for order in ORDERS:
        w5, w16 = P.expected_out5_rows(*c['terms'], order=order)
        out5, d16 = c[order]
        _same(out5[1:], w5, 'out5, %s order' % order)
        _same(d16[12:], w16, 'dict rows 12-15, %s order' % order)
    # what no order touches is the same in both
    assert np.array_equal(c['reference'][0][[0, 4]], c['record'][0][[0, 4]])
    assert np.array_equal(c['reference'][1][:12], c['record'][1][:12])


@pytest.mark.parametrize('task', TASKS)
def test_oracle_orders_equal_resum_on_rollout_inputs(oracle, task):
    for N, seed in ((VEH_NUM[task], 3), (16, 4), (64, 5)):
        inp = make_rollout_inputs(task, 500, N, 3, seed=seed, near_fraction=0.5)
        host = HostModel(oracle, task, n_veh=N)
        obs = initial_obs(host, inp)
        _held_to_resum(host, obs, inp['actions'][0], 'N = %d' % N)
        # the rollout twins form their sums in the same place: a step and a tape in order 1 against resum of each state
        host.set_penalty_order('record')
        out, o5s = host.rollout_tape(obs, inp['actions'], inp['ref_idx'])
        cur = obs
        for t in range(3):
            w5, _ = P.expected_out5_rows(*host.penalty_terms(cur), order='record')
            cur, o5, _ = host.rollout_step(cur, inp['actions'][t], inp['ref_idx'])
            _same(o5[1:], w5, 'rollout_step %d' % t)
            _same(o5s[t][1:], w5, 'rollout_tape step %d' % t)


def test_default_order_is_the_references(oracle):
    sc = P.scenes('left', 16, SEED)
    a, b = HostModel(oracle, 'left', n_veh=16), HostModel(oracle, 'left', n_veh=16, penalty_order='reference')
    c = HostModel(oracle, 'left', n_veh=16, penalty_order='record')
    o_a, o_b, o_c = (m.compute_rewards(sc['obs'], sc['actions'][0])[0] for m in (a, b, c))
    assert np.array_equal(o_a, o_b, equal_nan=True)
    assert not np.array_equal(o_a, o_c, equal_nan=True)          # (the dense rows)
    c.set_penalty_order('reference')                              # and the switch goes back
    assert np.array_equal(c.compute_rewards(sc['obs'], sc['actions'][0])[0], o_a, equal_nan=True)


@pytest.mark.parametrize('n_veh', SIZES)
@pytest.mark.parametrize('task', TASKS)
def test_order_free_rows(oracle, task, n_veh):
    """With at most two non-zero terms a sum has one value whatever the order (IEEE addition is commutative, x + 0 = x): the
    lone-pair and two-term blocks are such rows by construction — counted here from the exported terms — and penalised."""
    c = _case(oracle, task, n_veh)
    t35, t25, road = c['terms']
    for b in P.ORDER_FREE:
        if b not in c['rows']:
            assert c['N'] < 2 and b == 'two_records'
            continue
        r = c['rows'][b]
        n35, n25 = (t35[r] != 0).sum((1, 2)), (t25[r] != 0).sum((1, 2))
        assert np.all(road[r] == 0), b
        want = {'lone35': (1, 0), 'lone25': (1, 1), 'two_in_record': (2, None), 'two_records': (2, None)}[b]
        assert np.all(n35 == want[0]), '%s: %s terms under 3.5 m' % (b, sorted(set(n35)))
        if want[1] is not None:
            assert np.all(n25 == want[1]), '%s: %s terms under 2.5 m' % (b, sorted(set(n25)))
        assert np.all(n25 <= 2)
        assert np.array_equal(c['reference'][0][:, r], c['record'][0][:, r]), b
        assert np.array_equal(c['reference'][1][:, r], c['record'][1][:, r]), b
        assert np.all(c['record'][0][1, r] > 0), b
    # the lone pair is the pair asked for, in the slot asked for; slots cycle through all of them
    for b in ('lone35', 'lone25'):
        r = c['rows'][b]
        for i in r:
            pair, slot = c['meta'][i]
            assert t35[i, slot, P.PAIRS.index(pair)] > 0
        assert {c['meta'][i][1] for i in r} == set(range(c['N']))
        assert {c['meta'][i][0] for i in r} == set(P.PAIRS)
    assert np.any((t25[c['rows']['two_in_record']] != 0).sum((1, 2)) == 2)
    if 'two_records' in c['rows']:
        r = c['rows']['two_records']
        assert np.all((t35[r, 0] != 0).sum(1) == 1) and np.all((t35[r, c['N'] - 1] != 0).sum(1) == 1)


WORST = {}


@pytest.mark.parametrize('n_veh', SIZES)
@pytest.mark.parametrize('task', TASKS)
def test_orders_differ_on_dense_rows_within_the_derived_bound(oracle, task, n_veh):
    """Both orders add the same n non-negative float32 terms with n - 1 roundings each, every rounding at most 2^-24 of a partial
    sum that is at most the exact sum S: |a - S| <= (n - 1) 2^-24 S (1 + O(2^-24)) for either, so |a - b| <= 2 (n - 1) 2^-24 S.
    (S in float64 here; its own error and the second-order term are below 1e-6 of the bound.)"""
    c = _case(oracle, task, n_veh)
    t35, t25, road = c['terms']
    fin = ~np.isnan(c['record'][0]).any(0) & ~np.isnan(c['reference'][0]).any(0) & np.isfinite(t35).all((1, 2))
    worst = 0.0
    for terms, col, k in ((t35, 0, 1), (t25, 1, 2)):
        a, b = c['reference'][0][k].astype(np.float64), c['record'][0][k].astype(np.float64)
        n = (terms != 0).sum((1, 2)) + (road[:, col] != 0)
        S = terms.astype(np.float64).sum((1, 2)) + road[:, col].astype(np.float64)
        bound = 2.0 * np.maximum(n - 1, 0) * 2.0 ** -24 * S * (1 + 1e-6)
        assert np.all(np.abs(a - b)[fin] <= bound[fin])
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.where(fin & (S > 0), np.abs(a - b) / S, 0.0)
        worst = max(worst, float(rel.max()))
    dense = c['rows']['dense']
    differ = (c['reference'][0][1, dense] != c['record'][0][1, dense])
    assert differ.any(), 'no dense row tells the two orders apart: change the scene'
    WORST[(task, c['N'])] = worst
    print('penalty orders, %s N = %d: %d of %d dense rows differ, worst |reference - record| / sum = %.3e'
          % (task, c['N'], int(differ.sum()), len(dense), worst))
    assert worst < 2 * 4 * c['N'] * 2.0 ** -24


@pytest.mark.parametrize('n_veh', SIZES)
@pytest.mark.parametrize('task', TASKS)
def test_boundary_rows(oracle, task, n_veh):
    c = _case(oracle, task, n_veh)
    t35, t25, road = c['terms']
    r = c['rows']['boundary']
    cd = c['centre_distance'][r]
    assert np.all(road[r] == 0)
    beyond = r[cd >= 6.3 + 1e-3]
    assert len(beyond) >= 20 and np.all(t35[beyond] == 0) and np.all(t25[beyond] == 0)
    inside = r[cd < 6.3]
    tiny = (t35[inside] > 0) & (t35[inside] < 1e-8)
    assert tiny.any(), 'no term under 1e-8 just inside 3.5 m'
    tiny25 = (t25[r[cd < 5.3]] > 0) & (t25[r[cd < 5.3]] < 1e-8)
    assert tiny25.any(), 'no term under 1e-8 just inside 2.5 m'
    # only ego-front / vehicle-rear can be close on these rows
    assert np.all(t35[r][:, :, [0, 2, 3]] == 0)
    # both sides of the near filter's radius are there, and of each threshold
    assert (cd * cd < 40.5).any() and (cd * cd >= 40.5).any() and (cd < 5.3).any() and (cd > 5.3).any()


def test_walls_and_nonfinite_rows(oracle):
    for task in TASKS:
        c = _case(oracle, task, 16)
        t35, t25, road = c['terms']
        w = c['rows']['walls']
        assert np.all(road[w, 0] > 0)
        walls = np.array([c['meta'][i] for i in w])
        for k in set(walls):
            rows = w[walls == k]
            assert np.any(road[rows, 1] > 0) or (task == 'left' and k == 4)       # (the training-only wall of 'left')
            assert np.any((t35[rows] != 0).any((1, 2))) and np.any(~(t35[rows] != 0).any((1, 2)))   # `+ road` joins a sum and a zero
        others = np.setdiff1d(np.arange(len(road)), w)
        assert np.all(road[others] == 0)
        special = c['obs'][c['rows']['nonfinite']]
        with np.errstate(invalid='ignore'):
            assert np.all((~np.isfinite(special) | (np.abs(special) > 1e38)).any(1))


# ---- the reference's fixtures in order 1: still inside the fixture tolerance (order 0 stays what test_oracle_golden.py asserts) ----
TAG = '[record order] '
RTOL, ATOL = CK.RTOL, CK.ATOL


def _make_record(oracle):
    return lambda task, **kw: HostModel(oracle, task, penalty_order='record', **kw)


@pytest.mark.parametrize('task', TASKS)
def test_g3_and_g5t_fixtures_in_record_order(oracle, task):
    CK.check_g3_compute_rewards(_make_record(oracle), task, TAG)
    CK.check_g5t_teacher_forced_n32(_make_record(oracle), task, TAG)


G5 = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, 'g5_*.npz')))


@pytest.mark.parametrize('name', G5)
def test_g5_fixtures_in_record_order(oracle, name):
    _, _, task, N, mode, nf = name.split('_')
    g = golden(name)
    host = HostModel(oracle, task, n_veh=int(N[1:]), n_future=int(nf[2:]), mode=mode, modes=[str(m) for m in g['modes']],
                     penalty_order='record')
    obs = g['obs0']
    for t in range(g['actions'].shape[0]):
        obs, o5, _ = host.rollout_step(obs, g['actions'][t], g['ref_idx'], 1)
        close(o5, g['out5'][t], RTOL, ATOL['g5_closed_loop'], TAG + 'G5 closed loop x25: out5')
    if len(g['obs_step_index']) == g['actions'].shape[0]:
        states = [g['obs0']] + [g['obs_steps'][t] for t in range(g['actions'].shape[0])]
        for t in range(g['actions'].shape[0]):
            _, o5, _ = host.rollout_step(states[t], g['actions'][t], g['ref_idx'], 1)
            close(o5, g['out5'][t], RTOL, ATOL['g5_teacher'], TAG + 'G5 teacher-forced: out5 (native N)')


@pytest.mark.parametrize('task', TASKS)
def test_g8_fixture_in_record_order(oracle, task):
    g = golden('g8_fp16_rollout_%s_N64' % task)
    host = HostModel(oracle, task, n_veh=64, modes=[str(m) for m in g['modes']], penalty_order='record')
    for t in range(g['actions'].shape[0]):
        _, o5, _ = host.rollout_step_f16(g['obs_in'][t], g['actions'][t], g['ref_idx'])
        close(o5, g['out5'][t], RTOL, ATOL['g8'], TAG + 'G8 fp16 state: out5 (%s)' % task)


def test_record_order_fixture_margins_are_reported():
    """(runs after the fixture tests above: the figures DESIGN.md section 4 records)"""
    mine = {k: v for k, v in PARITY_LOG.items() if k.startswith(TAG)}
    for k in sorted(mine):
        print('%-70s excess %.3e  atol %.1e' % (k, mine[k][0], mine[k][1]))
    if WORST:
        print('worst |reference - record| / sum over all scenes: %.3e' % max(WORST.values()))
    assert all(ex <= atol for ex, atol in mine.values())


# ---- the switch itself ----
def test_set_penalty_order_refuses_unknown_orders_and_null(oracle):
    import ctypes as C
    host = HostModel(oracle, 'left')
    for bad in (2, -1, 7):
        with pytest.raises(ValueError, match='unknown order'):
            host.set_penalty_order(bad)
    assert host.penalty_order == 'reference'
    fn = oracle.lib.eb_oracle_set_penalty_order
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(None, 0) == -1 and fn(None, 1) == -1
    assert b'null handle' in oracle.lib.eb_last_error()
    # a refused call leaves the order as it was
    sc = P.scenes('left', 8, SEED)
    before = host.compute_rewards(sc['obs'], sc['actions'][0])[0]
    with pytest.raises(ValueError):
        host.set_penalty_order(5)
    assert np.array_equal(host.compute_rewards(sc['obs'], sc['actions'][0])[0], before, equal_nan=True)
    tf = oracle.lib.eb_oracle_penalty_terms
    tf.restype, tf.argtypes = C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    assert tf(None, 0, None, None, None, None) == -1
