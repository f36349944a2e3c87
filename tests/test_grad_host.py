"""CPU (-m "not gpu"): the gradient fixtures are self-consistent and G18 reaches every branch it was built for, the reverse pass's
arithmetic (csrc/eb_grad_device.h, run on the host) meets them, and — where the reference tree is present — the generator reproduces
them.  The ABI of include/envbuild_grad.h: tests/test_family_abi.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from env_build_amd import _capi
from tests._helpers import ROOT, build_host_harness, golden, _p
from tests._grad_cases import (TASKS, MAX_EXCLUDED, WALLS, cases, check_columns, check_zero_distance, edge_cases, edge_census,
                                step_and_edge_cases, zero_distance_case)


def test_differentiable_model_refuses_fp16_state():
    from env_build_amd.grad import DifferentiableEnvironmentModel
    with pytest.raises(_capi.EbError) as e:
        DifferentiableEnvironmentModel('left', state_dtype='float16')
    assert 'float16' in str(e.value) and 'reverse pass' in str(e.value)


@pytest.mark.parametrize('task', TASKS)
def test_gradient_fixtures_are_self_consistent(task):
    for kind in ('g15_grad_step', 'g16_grad_chain', 'g18_grad_edges'):
        path = os.path.join(ROOT, 'tests', 'golden', '%s_%s.npz' % (kind, task))
        assert os.path.getsize(path) <= 591861            # the largest fixture before these (g13_policy_left_2x256_elu.npz)
        cs = cases(kind, task)
        rows = sum(len(c['ok']) for c in cs)
        excluded = sum(int((~c['ok']).sum()) for c in cs)
        assert excluded <= MAX_EXCLUDED * rows, '%s %s: %d of %d rows excluded' % (kind, task, excluded, rows)
        assert {c.mode for c in cs} == {'training', 'selecting'} and {c.n_future for c in cs} == {0, 2}
        assert any(c.n_veh == 32 for c in cs)
        for c in cs:
            ok = c['ok']
            assert float(c['veh_grad_max']) == 0.0                        # stop_gradient: exactly zero in both precisions
            for g64, g32, E in ((c['g_obs64'], c['g_obs32'], c['E_obs']), (c['g_act64'], c['g_act32'], c['E_act'])):
                assert g64.dtype == np.float64 and g32.dtype == np.float32 and np.isfinite(g64).all()
                d = np.abs(g32.astype(np.float64) - g64)
                d = np.moveaxis(d, 0, 1).reshape(len(ok), -1, len(E)) if d.ndim == 3 else d.reshape(len(ok), 1, len(E))
                assert np.array_equal(d[ok].max((0, 1)), E)
            assert c['g_obs64'].shape == (len(ok), c.nd)
    assert any(c.n_veh == 64 for t in TASKS for c in cases('g15_grad_step', t))
    steps, chains = edge_cases(task)
    native = {'left': 8, 'straight': 9, 'right': 5}[task]
    assert {c.n_veh for c in steps} == {native, 32, 64} and {c.n_future for c in steps} == {0, 2}
    assert sorted((c.meta['horizon'], c.n_veh) for c in chains) == [(5, 32), (25, native)]


@pytest.mark.parametrize('task', TASKS)
def test_edge_fixtures_reach_every_branch(task):
    """G18's reason to exist, checked without trusting its generator: the branch conditions of DAM:129, 231-295, 390, 736-752 and the
    circle-centre distances, recomputed here in float64 NumPy from the stored obs / actions.  Every branch is taken by at least 8
    flagged rows of the task's step cases (a condition: enough that one excluded row cannot empty a branch), one 64-slot row has at
    least 48 near records, and where the generator's census (read off the reference's own float64 decision log) names the same
    branch the two counts are equal."""
    steps, _ = edge_cases(task)
    total, near64 = {}, 0
    for c in steps:
        took = edge_census(task, c)
        ok = c['ok']
        near = took.pop('near records')
        if c.n_veh == 64:
            near64 = max(near64, int(near[ok].max()))
        for name, rows in took.items():
            n = int((rows & ok).sum())
            total[name] = total.get(name, 0) + n
            if name in c.meta['census']:
                assert c.meta['census'][name] == n, (c.name, name)
        assert c.meta['census']['near vehicles in a row, max'] <= int(near[ok].max())     # a pair below 3.5 m is a near record
    print('\n'.join('g18 %-9s %-44s %4d' % (task, k, v) for k, v in sorted(total.items())))
    want = ['wall %s: %s' % (name, how) for name, _ in WALLS[task] for how in ('front', 'rear', 'both', 'far side', 'out of the region')]
    want += ['v_x below 0', 'v_x above 35', 'v_x just inside 0', 'v_x just inside 35', 'action clipped', 'crowded, 32 slots',
             'crowded, 64 slots', 'no vehicle near, 32 or 64 slots', 'ego off the cell grid', 'ego beyond 200 m', 'ego on the grid border',
             'ref_idx out of range']
    want += ['two2one before', 'two2one arc', 'two2one after'] if task != 'straight' else []
    assert sorted(want) == sorted(total)
    short = {k: v for k, v in total.items() if v < 8}
    assert not short, short
    assert near64 >= 48


@pytest.mark.parametrize('task', TASKS)
def test_fixture_forward_equals_the_rollout_fixtures(task):
    """The float32 run of the torch stand-in computes what the NumPy stand-in of the g5 fixtures computed: from the same state
    the rewards are the same bits; the penalty sums (sin / cos / sqrt of another libm) and the states of a chain agree to the
    tolerance every reference-generated fixture is held to here (rtol 1e-5 next to atol 5e-6, tests/test_gpu_parity.py)."""
    def near(a, b):
        return (np.abs(a.astype(np.float64) - b) <= 5e-6 + 1e-5 * np.abs(b)).all()
    n = 0
    for c in cases('g15_grad_step', task):
        steps = c.meta['g5_steps']
        if steps is None:
            continue
        z = golden('g5_rollout_%s_N%d_%s_nf%d' % (task, c.n_veh, c.mode, c.n_future))
        want = np.concatenate([z['out5'][t] for t in steps], 1)
        assert np.array_equal(c['out5_f32'][0], want[0]), c.name
        assert near(c['out5_f32'], want), c.name
        assert steps[0] != 0 or np.array_equal(c['obs'][:32], z['obs0'])
        n += 1
    for c in cases('g16_grad_chain', task):
        z = golden('g5_rollout_%s_N%d_%s_nf%d' % (task, c.n_veh, c.mode, c.n_future))
        assert np.array_equal(c['out5_f32'][0, 0], z['out5'][0, 0]), c.name
        assert near(c['out5_f32'], z['out5'][:c.meta['horizon']]), c.name
        assert np.array_equal(c['obs0'], z['obs0']) and np.array_equal(c['tape'], z['actions'][:c.meta['horizon']])
        n += 1
    assert n >= 8


@pytest.fixture(scope='module')
def host_harness(tmp_path_factory):
    """tests/_grad_host_harness.hip: the kernel's __host__ __device__ arithmetic compiled for the host"""
    return build_host_harness(tmp_path_factory, '_grad_host_harness.hip', 'grad_host')


def host_step_vjp(h, task, c, obs):
    obs, act = np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(c['actions'])
    n, D = obs.shape
    ri = c['ref_idx']
    has_path = np.ascontiguousarray(((ri >= 0) & (ri < 3)) if c.mode == 'training' else np.ones(n, bool), dtype=np.int32)
    g, g5 = np.ascontiguousarray(c['g_obs_out']), np.ascontiguousarray(c['g_out5'])
    go, ga = np.full((n, c.nd), np.nan, np.float32), np.full((n, 2), np.nan, np.float32)
    h.host_step_vjp(_capi.TASK_ID[task], n, D, c.nd, c.n_veh, c.n_future, _p(obs), _p(act), _p(has_path), _p(g), _p(g5), _p(go), _p(ga))
    return go, ga


@pytest.mark.parametrize('task', TASKS)
def test_reverse_pass_arithmetic_on_the_host_meets_the_step_fixtures(task, host_harness):
    for c in step_and_edge_cases(task):          # G15, and the step cases of G18
        go, ga = host_step_vjp(host_harness, task, c, c['obs'])
        check_columns(go, c['g_obs64'], c['E_obs'], c['ok'], 'host %s %s obs' % (task, c.name))
        check_columns(ga, c['g_act64'], c['E_act'], c['ok'], 'host %s %s act' % (task, c.name))


@pytest.mark.parametrize('task', TASKS)
def test_zero_circle_distance_contributes_nothing_and_stays_finite_on_the_host(task, host_harness):
    c, rows, obs, want = zero_distance_case(task)
    go, ga = host_step_vjp(host_harness, task, c, obs)
    check_zero_distance(c, rows, go, ga, want, 'host %s zero distance' % task)


def test_generator_reproduces_the_committed_fixtures():
    from oracle import refload
    if not refload.available():
        pytest.skip('reference tree not present (build container only)')
    # a process of its own: the torch stand-in has to be THE tensorflow module before the reference is imported
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'gen_golden_grad.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('reproduced') == 9
