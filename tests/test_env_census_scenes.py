"""CPU (the oracle alone): the scenes of the env rows of tests/_kernel_census (ENV_HELD, ENV_FEATURES) cannot pass vacuously.  Every
distinct seeded scene — a row kind or feature, a task, a batch of 2 ET + 3 envs; the tile and the waves change the launch, not the inputs —
runs through the oracle with the row's own case function and fixed parameters and meets: a flow row emits more vehicles than it has envs
and lets at least one exit (flow_rule_case's own `strict` condition, at the rows' 6 steps); an auto-reset, flow + auto-reset or time-limit
row finishes 2 .. 90 % of its envs (auto_reset_case's band), at least one in the first tile and one outside it; a masked reset masks an env
of the three-env tail.  These are conditions on the inputs, decided here and fixed in K.ENV_PARAMS; the GPU rows (tests/test_gpu_env_census.py)
run the same scenes."""
import numpy as np
import pytest

from tests import _env_census as EC, _kernel_census as K
from tests._helpers import HostModel, oracle_lib

SCENES = EC.distinct_scenes()


def test_the_scenes_are_one_per_kind_task_and_batch():
    assert len(SCENES) == 7 * 3 * 3 and {B for _, _, B in SCENES} == {35, 67, 131}
    assert {k for k, _, _ in SCENES} == set(K.ENV_PARAMS) == set(K.ENV_KINDS) | {'flow', 'flow_auto', 'time_limit'}
    for kind, rows in K.ENV_PARAMS.items():                          # an override names a scene that exists
        assert all(k is None or (kind,) + k in SCENES for k in rows), kind
    assert K.env_params('reset', 'left', 67) == dict(seed=23) and K.env_params('flow_auto', 'right', 67) == dict(steps=2, seed=15)
    assert K.env_params('flow', 'left', 35) == dict(steps=6, seed=3) and K.env_params('step', 'left', 35) == {}


@pytest.mark.parametrize('kind,task,B', SCENES, ids=['%s-%s-%d' % s for s in SCENES])
def test_the_scene_meets_its_conditions_on_the_oracle(kind, task, B):
    make = lambda t, **kw: HostModel(oracle_lib(), t, **kw)
    if kind == 'obs':
        sc = EC.obs_scene(task, B)
        ego, cand, cmode, light, ref, virtual = sc
        obs = make(task, mode='training').get_obs(ego, cand, cmode, light, ref_idx=ref, virtual=virtual)
        empty = make(task, mode='training').get_obs(ego, cand[:, :0], cmode[:, :0], light, ref_idx=ref, virtual=virtual)
        assert (obs != empty).any(1).mean() > 0.5                     # real candidates were selected into the rows' blocks
        EC.check_scene(kind, sc, B)
        return
    EC.check_scene(kind, EC.run_row(kind, make, task, B), B)


def test_the_conditions_reject_a_vacuous_scene():
    B, et = 35, 16
    none = [None] * 7 + [np.zeros(B, np.uint8)]
    with pytest.raises(AssertionError):
        EC.check_scene('auto', none, B)                              # nobody finishes
    first = [None] * 7 + [(np.arange(B) < 4).astype(np.uint8)]
    with pytest.raises(AssertionError, match='first tile'):
        EC.check_scene('time_limit', first, B)                       # only envs of the first tile finish
    outside = [None] * 7 + [(np.arange(B) >= et).astype(np.uint8) * 7]
    with pytest.raises(AssertionError, match='first tile'):
        EC.check_scene('auto', outside, B)
    both = [None] * 7 + [np.isin(np.arange(B), (2, 20)).astype(np.uint8)]
    EC.check_scene('auto', both, B)
    EC.check_scene('flow_auto', [both, none], B)                     # over a trace: some step finishes in each part
    code = np.full(B, 7, np.uint8)
    code[:5] = 0
    with pytest.raises(AssertionError):
        EC.check_scene('reset', [[None] * 5 + [code]], B)            # the mask misses the ragged tail
    code[-1] = 0
    EC.check_scene('reset', [[None] * 5 + [code]], B)
