"""CPU (-m "not gpu"): the closed-loop gradient fixtures G21 (scripts/gen_golden_policy_grad.py) are what their GPU test takes them
for — present, small, every row meeting the generator's conditions, the float32 run of the reference within rounding noise of the
float64 one — and their float32 forward is the CPU oracle's policy -> rollout_step loop, so that a disagreement between generator and
project about the obs scale, action_range or the mode shows without a GPU.  Where the reference tree is present the generator
reproduces them."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from env_build_amd.policy_sample import policy_sample_reference
from tests import _policy
from tests import _policy_rollout_fixture as F
from tests._helpers import GOLDEN, ROOT, HostModel, close, golden, oracle_lib

NATIVE = {'left': 8, 'straight': 9, 'right': 5}


@pytest.mark.parametrize('task', F.TASKS)
def test_fixtures_are_present_small_and_self_consistent(task):
    path = os.path.join(GOLDEN, F.stem(task) + '.npz')
    assert os.path.getsize(path) <= F.MAX_BYTES
    cs = F.cases(task)
    assert [c.name for c in cs] == ['det_H5', 'sto_H5', 'det_sel_H3'] + (['det_H1_N32'] if task == 'left' else [])
    want = {'det_H5': ('eb_policy_rollout_grad', 'training', 5, 1.0, False, 2, 'elu', True, 96, NATIVE[task]),
            'sto_H5': ('eb_policy_rollout_sample', 'training', 5, 1.0, True, 2, 'elu', True, 96, NATIVE[task]),
            'det_sel_H3': ('eb_policy_rollout_grad', 'selecting', 3, 0.5, False, 1, 'tanh', False, 96, NATIVE[task]),
            'det_H1_N32': ('eb_policy_rollout_grad', 'training', 1, 1.0, False, 2, 'elu', True, 32, 32)}
    for c in cs:
        m = c.meta
        assert (c.entry, c.mode, c.steps, c.ar, c.sampled, m['n_hidden'], c.hact, m['obs_scale'], c.n, c.n_veh) == want[c.name], c.name
        assert m['units'] == 64 and m['n_future'] == 0 and c.D == 9 + 4 * c.n_veh and c.obs0.dtype == np.float32
        assert c['ok'].shape == (c.n,) and c['ok'].all(), '%s: g_params sums over every row, none may fail a condition' % c.name
        assert (c.scale is not None) == m['obs_scale'] and (c.scale is None or ((c.scale >= 0.05) & (c.scale <= 0.3)).all())
        assert np.abs(c['actions_steps']).max() < 1.05                          # DAM:129's clip is inactive
        steps, n = c.steps, c.n
        for key, shape in (('out5_steps', (steps, 5, n)), ('actions_steps', (steps, n, 2)), ('g_obs0_64', (n, 9)),
                           ('g_actions_steps_64', (steps, n, 2)), ('E_obs0', (9,)), ('E_actions', (2,)), ('E_params', (len(c.weights),))):
            assert c[key].shape == shape, (c.name, key)
        if c.sampled:
            assert c.eps.shape == (steps, n, 2) and c['logp_steps'].shape == (steps, n) and c.w_logp == np.float32(0.3 / (steps * n))
            lo, hi = c['log_std_range']
            assert -2.0 <= lo <= hi <= 1.0 and float(c['x_abs_max']) <= 6.0     # tests/test_gpu_ppo.py's bounds on its twin
        else:
            assert c.w_logp == 0.0
        # E is what it says, and the float32 run has not diverged: 4 E below 1e-4 of each tensor's (column's) maximum
        pairs = [(c['g_obs0_64'], c['g_obs0_32'], c['E_obs0'], 9), (c['g_actions_steps_64'], c['g_actions_steps_32'], c['E_actions'], 2)]
        pairs += [(c['g_params_64_%d' % k], c['g_params_32_%d' % k], c['E_params'][k:k + 1], 1) for k in range(len(c.weights))]
        for g64, g32, E, cols in pairs:
            assert g64.dtype == np.float64 and g32.dtype == np.float32 and g64.shape == g32.shape and np.isfinite(g64).all()
            assert np.array_equal(np.abs(g32.astype(np.float64) - g64).reshape(-1, cols).max(0), E)
            top = np.abs(g64).reshape(-1, cols).max(0)
            assert (top > 0).all() and (4.0 * E < 1e-4 * top).all(), (c.name, E / top)
        for k, w in enumerate(c.weights):
            assert c['g_params_64_%d' % k].shape == w.shape and w.dtype == np.float32
        if not c.sampled:
            # d J / d obs0 is not zero on the vehicle columns — the policy reads them at step 0 — which is why the header's g_obs0
            # is defined as the nine ego and tracking columns and the fixture compares those
            assert float(c['veh_grad_max']) > 0.0
    assert 'reference' in str(golden(F.stem(task))['note'])


@pytest.mark.parametrize('c', F.all_cases(), ids=F.case_id)
def test_float32_forward_is_the_oracles_policy_and_rollout_step_loop(c):
    """rtol 1e-5 next to atol 5e-6: what every reference-generated fixture's forward is held to (tests/test_gpu_parity.py)"""
    host = HostModel(oracle_lib(), c.task, n_veh=c.n_veh, mode=c.mode)
    assert host.D == c.D
    m = host.make_mlp(*c.net_args())
    what = 'G21 %s %s oracle ' % (c.task, c.name)
    if not c.sampled:
        got = _policy.loop(host, m, c.obs0, c.steps, c.ref_idx(), c.path_id(), c.ar)
    else:
        obs, got = c.obs0, {'out5': [], 'actions': [], 'logp': []}
        for t in range(c.steps):
            a, lp, _ = policy_sample_reference(host.mlp_forward(m, 4, obs), c.eps[t], c.ar)
            obs, out5, _ = host.rollout_step(obs, a, c.ref_idx(), c.path_id())
            got['out5'].append(out5); got['actions'].append(a); got['logp'].append(lp)
        got = {k: np.stack(v) for k, v in got.items()}
        close(got['logp'], c['logp_steps'], F.RTOL, F.ATOL, what + 'logp')
    close(got['actions'], c['actions_steps'], F.RTOL, F.ATOL, what + 'actions')
    close(got['out5'], c['out5_steps'], F.RTOL, F.ATOL, what + 'out5')
    host.api.mlp_destroy(m)


def test_nothing_in_the_package_or_the_gpu_tests_imports_the_generator():
    for f in glob.glob(os.path.join(ROOT, 'env_build_amd', '**', '*.py'), recursive=True) + glob.glob(os.path.join(ROOT, 'tests', 'test_gpu_*.py')):
        with open(f) as fh:
            assert not re.search(r'^\s*(import|from)\s+\S*gen_golden_policy_grad', fh.read(), re.M), f


def test_generator_reproduces_the_committed_fixtures():
    from oracle import refload
    if not refload.available():
        pytest.skip('reference tree not present (build container only)')
    # a process of its own: the torch stand-in has to be THE tensorflow module before the reference is imported
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'gen_golden_policy_grad.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('reproduced') == 3
