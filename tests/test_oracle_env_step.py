"""CPU (-m "not gpu"): the oracle's eb_env_step composite (incl. the re-entry rule, the nullable outputs and ABI 4's auto_reset)
equals its own single calls — the same check the GPU suite runs on the one-launch kernel (tests/_env_step_check.py)."""
import pytest

from tests._env_step_check import (CASES, auto_reset_bad_args_case, auto_reset_case, composite_case, flow_rule_bad_args_case,
                                   flow_auto_reset_case, flow_rule_case, g20_parked_auto_reset_case, g20_parked_case, g20_parked_flow_case,
                                   masked_obs_case, parked_ego_case, reset_pool_case, respawn_conflict_case, time_limit_case, wrap_guard_case)
from tests._helpers import HostModel


@pytest.mark.parametrize('task,B,M,NV,nf', CASES[3:7])
def test_oracle_env_step_composite(oracle, task, B, M, NV, nf):
    composite_case(lambda t, **kw: HostModel(oracle, t, **kw), task, B, M, NV, nf)


@pytest.mark.parametrize('widened', [False, True], ids=['native', 'N16'])
@pytest.mark.parametrize('task', ['left', 'straight', 'right'])
def test_oracle_env_step_on_the_parked_g20_scenes(oracle, task, widened):
    """fixture G20's families A-D, parked, through the composite: the positions come through with their input bits (no allowance), the
    composite equals the six calls, and its block's x, y, v columns equal the reference's"""
    g20_parked_case(lambda t, **kw: HostModel(oracle, t, **kw), task, widened=widened)


@pytest.mark.parametrize('widened', [False, True], ids=['native', 'N16'])
@pytest.mark.parametrize('task', ['left', 'straight', 'right'])
def test_oracle_auto_reset_and_flow_rule_on_the_parked_g20_scenes(oracle, task, widened):
    g20_parked_auto_reset_case(lambda t, **kw: HostModel(oracle, t, **kw), task, widened=widened)
    g20_parked_flow_case(lambda t, **kw: HostModel(oracle, t, **kw), task, widened=widened)


@pytest.mark.parametrize('task', ['left', 'straight', 'right'])
def test_oracle_masked_observation_pass(oracle, task):
    masked_obs_case(lambda t, **kw: HostModel(oracle, t, **kw), task)


def test_oracle_pool_reset_keeps_clear_of_the_ego(oracle):
    respawn_conflict_case(lambda t, **kw: HostModel(oracle, t, **kw))


@pytest.mark.parametrize('task', ['left', 'straight', 'right'])
def test_oracle_reset_pool_composite(oracle, task):
    reset_pool_case(lambda t, **kw: HostModel(oracle, t, **kw), task)


@pytest.mark.parametrize('task,B,M,NV,nf,vln', [('left', 300, 16, None, 0, False), ('straight', 200, 10, None, 1, False),
                                                 ('right', 130, 20, 7, 0, True)])
def test_oracle_step_with_auto_reset(oracle, task, B, M, NV, nf, vln):
    """ABI 4: eb_env_step(auto_reset) == eb_env_step + terminal rows + eb_env_reset_pool(mask = done != 0)"""
    auto_reset_case(lambda t, **kw: HostModel(oracle, t, **kw), task, B, M, NV=NV, nf=nf, v_light_none=vln)


@pytest.mark.parametrize('task,B,M', [('left', 400, 16), ('right', 130, 20)])
def test_oracle_step_with_the_episode_step_limit(oracle, task, B, M):
    """ABI 5: eb_time_limit = gym's TimeLimit around the registered env (README.md:55-59, max_episode_steps = 200)"""
    time_limit_case(lambda t, **kw: HostModel(oracle, t, **kw), task, B, M)


def test_oracle_parked_ego_is_truncated_at_the_step_limit(oracle):
    parked_ego_case(lambda t, **kw: HostModel(oracle, t, **kw))


def test_oracle_auto_reset_argument_checks(oracle):
    auto_reset_bad_args_case(lambda t, **kw: HostModel(oracle, t, **kw))


@pytest.mark.parametrize('task,K', [('left', 5), ('right', 2)])
def test_oracle_step_with_the_flow_rule(oracle, task, K):
    """ABI 4: eb_env_step(flow) == eb_env_step + eb_traffic_flow_step over a closed loop"""
    flow_rule_case(lambda t, **kw: HostModel(oracle, t, **kw), task, B=120, K=K, steps=30)


def test_oracle_flow_rule_on_records_no_source_would_make(oracle):
    """the composite and the two calls agree on far-out records at any heading, many-turn headings, box-to-far jumps, NaN / inf fields
    (the inputs of the GPU test of the same name)"""
    flow_rule_case(lambda t, **kw: HostModel(oracle, t, **kw), 'left', B=120, K=5, steps=3, strict=False, hostile=True)


@pytest.mark.parametrize('task,K', [('left', 5), ('right', 2)])
def test_oracle_step_with_the_flow_rule_and_auto_reset(oracle, task, K):
    """ABI 5: eb_env_step(flow + auto_reset) == eb_env_step(flow) + eb_env_reset + eb_traffic_flow_reset + eb_get_obs(mask) + flag swap"""
    flow_auto_reset_case(lambda t, **kw: HostModel(oracle, t, **kw), task, B=120, K=K, steps=8)


def test_oracle_flow_rule_argument_checks(oracle):
    flow_rule_bad_args_case(lambda t, **kw: HostModel(oracle, t, **kw))


@pytest.mark.timeout(60)
def test_angle_wrap_loops_are_bounded(oracle):
    wrap_guard_case(HostModel(oracle, 'left'))


def test_reset_pool_refuses_a_mask_that_is_an_output(oracle):
    """include/envbuild.h: the mask may be the previous done codes, but not the array the new ones are written to"""
    import ctypes as C
    import numpy as np
    from env_build_amd import _capi
    B, M = 8, 4
    m = HostModel(oracle, 'left', mode='training')
    tr = HostModel(oracle, 'left', n_veh=M, modes=['dl', 'du', 'ud', 'ul'])
    f32 = lambda *s: np.zeros(s, np.float32)
    ego, params, ref, virt, vl, done = f32(B, 6), f32(B, 4), np.zeros(B, np.int32), np.zeros(B, np.uint8), np.zeros(B, np.uint8), np.ones(B, np.uint8)
    cand, cmode, obs, entry = f32(B, M, 4), np.zeros((B, M), np.uint8), f32(B, m.D), f32(M, 5)
    rule = _capi.EbRespawn(entry.ctypes.data, 0.0, 60.0, 8.0, 1, 1, 5.0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    args = lambda mask, dc: (m.h, tr.h, B, p(mask), C.c_uint64(1), C.c_uint64(1), 1, p(ego), p(params), p(ref), p(virt), p(vl), p(dc), None, M, p(cand),
                             p(cmode), C.byref(rule), p(obs), None, None, None)
    with pytest.raises(ValueError, match='mask must not be'):          # EB_EINVAL surfaces as ValueError (_capi.check)
        oracle.env_reset_pool(*args(done, done))
    fresh = np.full(B, 7, np.uint8)
    oracle.env_reset_pool(*args(done, fresh))                # the done codes as the mask, a fresh array for the new ones
    assert (fresh == 0).all()
