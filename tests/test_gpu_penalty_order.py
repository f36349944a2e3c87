"""GPU: the penalty sums of every path that forms them, on the scenes of tests/_penalty.py, bit for bit against the oracle summing
in the kernels' order (penalty_order='record'; the oracle's switch is held to an independent restatement by
tests/test_penalty_order_host.py).  The scenes hold what a relative tolerance cannot see: one tiny term beside nothing, one slot
(bit 63 of the slot mask included) whose partial is the whole sum, distances within float32 steps of the 3.5 m / 2.5 m thresholds and of
the near filter's radius, dense rows on which another association gives other bits, `+ road`, non-finite records.

Each test prints how many rows carry a non-zero sum, per block of the scene."""
import numpy as np
import pytest

from env_build_amd import _capi
from env_build_amd.endtoend_env_utils import VEH_NUM, VEHICLE_MODE_LIST, tiled_mode_list
from tests import _penalty as P
from tests._helpers import DeviceModel, bits_equal, check_out5, check_out5_steps, record_host
from tests._policy_cases import make_layers

pytestmark = pytest.mark.gpu
SEED = 20                                        # (tests/test_penalty_order_host.py holds the scenes' properties at this seed)
ALL = [(t, n) for t in ('left', 'straight', 'right') for n in ('native', 16, 64)]
SOME = [('left', 'native'), ('straight', 16), ('right', 64), ('left', 64)]
H = 3
_cache = {}


def _case(task, n_veh):
    """the scene, both models and the oracle's answers shared by the tests of (task, n_veh) — computed once, never written to"""
    N = VEH_NUM[task] if n_veh == 'native' else n_veh
    if (task, N) not in _cache:
        sc = P.scenes(task, N, SEED)
        host, dev = record_host(task, n_veh=N), DeviceModel(task, n_veh=N)
        obs, ri = sc['obs'], sc['ref_idx']
        want = dict(rewards=host.compute_rewards(obs, sc['actions'][0]))
        cur, steps = obs, []
        for t in range(H):
            cur, o5, _ = host.rollout_step(cur, sc['actions'][t], ri)
            steps.append(o5)
        want['steps'], want['last'] = np.stack(steps), cur
        for a in list(want['rewards']) + [want['steps'], want['last']]:
            a.setflags(write=False)
        _cache[(task, N)] = dict(sc, N=N, task=task, host=host, dev=dev, want=want)
    return _cache[(task, N)]


def _report(c, path, o5):
    """one line per path: rows with a non-zero punish_train per block; the order-free blocks must be penalised on every row"""
    o5 = np.asarray(o5)
    with np.errstate(invalid='ignore'):
        hit = ~(o5[1] == 0)
    line = ', '.join('%s %d/%d' % (b, int(hit[r].sum()), len(r)) for b, r in c['rows'].items())
    print('%s [%s N = %d]: rows with a non-zero sum: %d of %d (%s)' % (path, c['task'], c['N'], int(hit.sum()), hit.size, line))
    for b in P.ORDER_FREE:
        if b in c['rows']:
            assert hit[c['rows'][b]].all(), '%s: a row of %s without a penalty' % (path, b)


@pytest.mark.parametrize('task,n_veh', ALL)
def test_compute_rewards_and_dict(task, n_veh):
    c = _case(task, n_veh)
    o5, d16 = c['dev'].compute_rewards(c['obs'], c['actions'][0])
    w5, w16 = c['want']['rewards']
    check_out5(o5, w5, 'eb_compute_rewards', exact=True)
    bits_equal(d16, w16, 'the reward dictionary')
    _report(c, 'eb_compute_rewards', o5)
    walls = c['rows']['walls']
    assert (d16[13, walls] > 0).all() and (np.delete(d16[13], walls) == 0).all()        # `+ road` only where a wall is


@pytest.mark.parametrize('tile', [0, 1, 2])
@pytest.mark.parametrize('task,n_veh', ALL)
def test_rollout_step_tiles(task, n_veh, tile):
    c = _case(task, n_veh)
    dev = c['dev']
    dev.set_tile(tile)
    try:
        assert dev.rollout_plan(len(c['obs']))[0] == tile
        out, o5, _ = dev.rollout_step(c['obs'], c['actions'][0], c['ref_idx'])
    finally:
        dev.set_tile(-1)
    check_out5(o5, c['want']['steps'][0], 'rollout_step, tile %d' % tile, exact=True)
    _report(c, 'rollout_step tile %d' % tile, o5)


@pytest.mark.parametrize('rolling,by_progress', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('task,n_veh', SOME)
def test_rollout_step_schedules(task, n_veh, rolling, by_progress):
    c = _case(task, n_veh)
    dev = c['dev']
    dev.set_tile(0)
    dev.set_rollout_sched(rolling, by_progress)
    try:
        assert dev.rollout_plan(len(c['obs']))[2:] == (rolling, by_progress)
        out, o5, _ = dev.rollout_step(c['obs'], c['actions'][0], c['ref_idx'])
    finally:
        dev.set_rollout_sched(-1, -1)
        dev.set_tile(-1)
    check_out5(o5, c['want']['steps'][0], 'rollout_step, rolling %d, by progress %d' % (rolling, by_progress), exact=True)
    _report(c, 'rollout_step rolling %d by_progress %d' % (rolling, by_progress), o5)


@pytest.mark.parametrize('task,n_veh', SOME)
def test_rollout_step_f16(task, n_veh):
    c = _case(task, n_veh)
    with np.errstate(over='ignore'):
        obs16 = c['obs'].astype(np.float16).view(np.uint16)
    out_h, o5_h, _ = c['host'].rollout_step_f16(obs16, c['actions'][0], c['ref_idx'])
    out_d, o5_d, _ = c['dev'].rollout_step_f16(obs16, c['actions'][0], c['ref_idx'])
    check_out5(o5_d, o5_h, 'rollout_step_f16', exact=True)
    assert (o5_h[1, c['rows']['dense']] > 0).all()
    print('rollout_step_f16 [N = %d]: rows with a non-zero sum: %d of %d' % (c['N'], int((o5_d[1] != 0).sum()), o5_d.shape[1]))


@pytest.mark.parametrize('tile', [-1, 0, 1, 2])
@pytest.mark.parametrize('task,n_veh', SOME)
def test_rollout_tape_every_step(task, n_veh, tile):
    c = _case(task, n_veh)
    dev = c['dev']
    dev.set_tile(tile)
    try:
        out, o5 = dev.rollout_tape(c['obs'], c['actions'][:H], c['ref_idx'])
    finally:
        dev.set_tile(-1)
    for t in range(H):
        check_out5(o5[t], c['want']['steps'][t], 'rollout_tape tile %d, step %d' % (tile, t), exact=True)
    _report(c, 'rollout_tape tile %d' % tile, o5[0])


@pytest.mark.parametrize('task,n_veh', SOME)
def test_gated_rollout_with_open_gates(task, n_veh):
    c = _case(task, n_veh)
    out, o5, _, done, status = c['dev'].rollout_gated(c['obs'], c['actions'][:H], c['ref_idx'], publish_obs=False)
    assert status.tolist() == [0, 0] and done.all()
    check_out5_steps(o5, c['want']['steps'], exact=True)
    _report(c, 'rollout_gated', o5[0])


@pytest.mark.parametrize('tile', [0, 1, 2])
@pytest.mark.parametrize('task,n_veh', SOME)
def test_env_step_composite(task, n_veh, tile):
    """the scene's vehicles as the candidate pool, one candidate per slot: the step's penalty sums are those of the rows it is given"""
    c = _case(task, n_veh)
    N, B = c['N'], len(c['obs'])
    native = VEHICLE_MODE_LIST[task]
    modes = list(native) if N == len(native) else list(tiled_mode_list(task, N))
    cmode = np.tile(np.array([_capi.VMODE_ID[m] for m in modes], np.uint8), (B, 1))
    ego, cand = c['obs'][:, :6].copy(), c['obs'][:, 9:].reshape(B, N, 4).copy()
    raw = c['actions'][1]
    light, virtual = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    res = []
    for make, tl in ((record_host, None), (DeviceModel, tile)):
        m, tr = make(task, n_veh=N), make(task, n_veh=N, modes=modes)
        if tl is not None:
            m.set_tile(tl)
        res.append(m.env_step(tr, c['obs'], raw, ego, cand, cmode, ref_idx=c['ref_idx'], v_light=light, virtual=virtual))
    (sc_h, o5_h, d16_h), (sc_d, o5_d, d16_d) = res[0][:3], res[1][:3]
    assert np.array_equal(sc_d, sc_h)
    check_out5(o5_d, o5_h, 'eb_env_step, tile %d' % tile, exact=True)
    bits_equal(d16_d, d16_h, 'eb_env_step: the reward dictionary')
    # the same rows, so the same sums as eb_compute_rewards on them
    bits_equal(o5_h[1:], c['host'].compute_rewards(c['obs'], sc_h)[0][1:], 'the oracle\'s composite against its compute_rewards')
    _report(c, 'eb_env_step tile %d' % tile, o5_d)


@pytest.mark.parametrize('penalty,steps', [(0, 3), (1, 3), (1, 1)])
@pytest.mark.parametrize('task,n_veh', SOME)
def test_shield_punish(task, n_veh, penalty, steps):
    c = _case(task, n_veh)
    host, dev = c['host'], c['dev']
    rng = np.random.default_rng(c['N'])
    net = (host.D, 2, 64, 4, 'elu', 'linear', make_layers(rng, host.D, 2, 64, 4), rng.uniform(0.02, 0.2, host.D).astype(np.float32))
    mh, md = host.make_mlp(*net), dev.make_mlp(*net)
    try:
        fin = np.isfinite(c['obs']).all(1) & (np.abs(c['obs']) < 1e30).all(1)    # (a network fed inf / NaN is tests/test_gpu_policy.py's subject)
        obs = c['obs'][fin]
        want = host.shield_is_safe(mh, obs, ref_idx=c['ref_idx'][fin], steps=steps, penalty=penalty)
        got = dev.shield_is_safe(md, obs, ref_idx=c['ref_idx'][fin], steps=steps, penalty=penalty)
    finally:
        host.api.mlp_destroy(mh); dev.api.mlp_destroy(md)
    bits_equal(got[1], want[1], 'punish (penalty %d, %d steps)' % (penalty, steps))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    print('eb_shield_is_safe penalty %d, %d steps [N = %d]: rows with a non-zero sum: %d of %d'
          % (penalty, steps, c['N'], int((got[1] != 0).sum()), len(obs)))
    assert (got[1][:len(c['rows']['lone35']) + len(c['rows']['lone25'])] > 0).sum() >= len(c['rows']['lone25'])
