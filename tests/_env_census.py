"""The rows of tests/_kernel_census.ENV_HELD / ENV_FEATURES as calls of the case functions of tests/_env_step_check.py, and the
conditions a row's scene has to meet so that the row cannot pass vacuously.  A helper module: pytest does not collect it, and importing
it touches no device.  tests/test_env_census_scenes.py runs every distinct scene through the oracle alone and holds the conditions;
tests/test_gpu_env_census.py runs the rows on the device with the tile and the waves per block forced."""
import numpy as np

from tests import _kernel_census as K


def run_row(kind, make, task, B, tile=None, waves=None):
    """the case function of a row kind / feature at the row's batch, with the row's fixed parameters (K.ENV_PARAMS) -> its result"""
    from tests import _env_step_check as E
    p = K.env_params(kind, task, B)
    if kind == 'step':
        return E.composite_case(make, task, B, K.ENV_CAND, None, 0, tile=tile, waves=waves)
    if kind == 'auto':
        return E.auto_reset_case(make, task, B, K.ENV_CAND, tile=tile, waves=waves, **p)
    if kind == 'reset':
        return E.reset_pool_case(make, task, B=B, M=K.ENV_CAND, tile=tile, waves=waves, **p)
    if kind == 'flow':
        return E.flow_rule_case(make, task, B=B, K=K.FLOW_K, tile=tile, waves=waves, **p)
    if kind == 'flow_auto':
        return E.flow_auto_reset_case(make, task, B=B, K=K.FLOW_K, tile=tile, waves=waves, **p)
    assert kind == 'time_limit', kind
    return E.time_limit_case(make, task, B, K.ENV_CAND, tile=tile, waves=waves, **p)


def obs_scene(task, B):
    """the scene of an observation row: eb_get_obs over random_scene's candidates -> (ego, cand, cmode, light, ref, virtual)"""
    from tests._env_step_check import random_scene
    ego, cand, cmode, _, light, _, ref = random_scene(task, B, K.ENV_CAND, 300 + B)
    virtual = (np.random.default_rng(B).random(B) < 0.3).astype(np.uint8)
    return ego, cand, cmode, light, ref, virtual


def finished(kind, result):
    """[steps, B] bool: the envs each step of an auto-reset / time-limit row finished (done_code != 0)"""
    if kind == 'flow_auto':
        return np.stack([np.asarray(g[7]) != 0 for g in result])
    return (np.asarray(result[7]) != 0)[None]


def check_scene(kind, result, B):
    """the conditions on a row's scene, from the ORACLE's result of run_row (the case functions assert their own `strict` conditions
    while they run: a flow row emits more vehicles than it has envs and lets one exit; an auto-reset row finishes 2 .. 90 % of its envs;
    a time-limit row truncates some envs, finishes some by a predicate and leaves some running)"""
    et = (B - 3) // 2
    if kind in ('auto', 'flow_auto', 'time_limit'):
        fin = finished(kind, result)
        frac = float(fin.mean())
        assert 0.02 < frac < 0.9, (kind, B, frac)
        assert fin[:, :et].any() and fin[:, et:].any(), (kind, B, 'no finished env in the first tile / outside it')
    elif kind == 'reset':
        masked = np.asarray(result[0][5]) == 0                       # done_code: 0 on the masked rows, the 7 it held elsewhere
        assert masked[-3:].any() and not masked.all() and masked[:et].any(), (kind, B, masked[-3:])
    elif kind == 'obs':
        ego, cand, cmode, light, ref, virtual = result
        assert len(ego) == B and cand.shape == (B, K.ENV_CAND, 4)
    else:
        assert kind in ('step', 'flow'), kind


def distinct_scenes():
    """[(kind or feature, task, B)] — a row's scene depends on nothing else (the tile and the waves change the launch, not the inputs)"""
    seen = []
    for _, kind, key, case in K.env_rows():
        s = (kind, case.task, K.env_batch_of(case))
        if s not in seen:
            seen.append(s)
    return seen
