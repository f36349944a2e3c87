"""GPU (-m gpu): fixture G20 (oracle/gen_golden_env_edges.py — filter bounds on / one ulp inside / one ulp outside, sort ties the
slice cuts, the stop-line car, counts, done rules, walls, stability, the priority chain, the collision circles; the reference's
recorded outputs) through every implementation of the env-side selection in the HIP library:

  get_obs_kernel (veh_in_range / veh_cmp), staged / per thread   test_g20_env_edges_on_gpu[separate_staged], [separate_unstaged]: eb_get_obs
                                                                 with a misaligned ego / candidate array (an aligned call of up to 64
                                                                 candidates takes the one-launch observation kernel instead)
  get_obs_exit_kernel (veh_in_range_d / veh_cmp_d)               test_g20_env_edges_on_gpu[exit0]
  slot_pair_walk<TASK, MODE> (at most two slots of a mode)       test_g20_env_edges_on_gpu[native-single], [native-masked] (the one-launch
                                                                 observation kernel); ..._through_the_one_launch_step[native-tile0 / tile1]
  the selection pass (more than two slots of a mode)             test_g20_env_edges_on_gpu[N16-single], [N16-masked];
                                                                 ..._through_the_one_launch_step[N16-*], ..._auto_reset_and_the_flow_rule[N16-*]
  range_box / box_in_range / key_of / key_before walk            ..._through_the_one_launch_step[native-tile2], [native-default] (16-env tiles);
                                                                 ..._with_auto_reset_and_the_flow_rule[native-*] (the auto-reset tail)
  eb_judge_done's own kernel                                     test_g20_env_edges_on_gpu[*-single]
The CPU suite replays the same checks on the oracle (tests/test_oracle_golden.py, tests/test_oracle_env_step.py); the census of what
the fixture holds is tests/test_env_edges_census.py."""
import numpy as np
import pytest

from tests import _golden_checks as CK
from tests._env_step_check import g20_parked_auto_reset_case, g20_parked_case, g20_parked_flow_case
from tests._helpers import DeviceModel, bits_equal, record_host

pytestmark = pytest.mark.gpu
TASKS = ('left', 'straight', 'right')
TAG = '[gpu] '
WIDE = pytest.mark.parametrize('widened', [False, True], ids=['native', 'N16'])


def _gpu(task, **kw):
    return DeviceModel(task, **kw)


def _cpu(task, **kw):
    return record_host(task, **kw)


def _same_as_oracle(got, want, what):
    """the HIP library's outputs against the oracle's: bit for bit (headings included; the penalty sums too: the oracle adds them in the kernels' order)"""
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (what, k)
        elif np.asarray(w).dtype == np.float32 and np.asarray(w).ndim == 2 and np.asarray(w).shape[0] in (5, 16):
            bits_equal(g, w, '%s output %d' % (what, k))
        else:
            assert np.array_equal(g, w, equal_nan=True), (what, k)


@pytest.mark.parametrize('form', ['single', 'exit0', 'masked', 'separate_staged', 'separate_unstaged'])
@WIDE
@pytest.mark.parametrize('task', TASKS)
def test_g20_env_edges_on_gpu(task, widened, form):
    (CK.check_g20w_env_edges if widened else CK.check_g20_env_edges)(_gpu, task, TAG, form=form)


@pytest.mark.parametrize('tile', [None, 0, 1, 2], ids=['default', 'tile0', 'tile1', 'tile2'])
@WIDE
@pytest.mark.parametrize('task', TASKS)
def test_g20_parked_scenes_through_the_one_launch_step(task, widened, tile):
    got = g20_parked_case(_gpu, task, tile=tile, widened=widened)
    _same_as_oracle(got, g20_parked_case(_cpu, task, widened=widened), 'G20 parked step')


@pytest.mark.parametrize('tile', [None, 2], ids=['default', 'tile2'])
@WIDE
@pytest.mark.parametrize('task', TASKS)
def test_g20_parked_scenes_with_auto_reset_and_the_flow_rule(task, widened, tile):
    got = g20_parked_auto_reset_case(_gpu, task, tile=tile, widened=widened)
    _same_as_oracle(got, g20_parked_auto_reset_case(_cpu, task, widened=widened), 'G20 parked auto reset')
    got = g20_parked_flow_case(_gpu, task, tile=tile, widened=widened)
    _same_as_oracle(got[0], g20_parked_flow_case(_cpu, task, widened=widened)[0], 'G20 parked flow rule')
