"""CPU (-m "not gpu"): the one-launch value and gradient of an open-loop rollout (eb_rollout_tape_vjp: the entries envbuild_grad.h gained
with its version 2; the header as a family: tests/test_family_abi.py) is declared, bound and exported; a library without it is refused
cleanly; its per-env reverse sweep (csrc/eb_tape_grad_device.h, the text the kernel runs, compiled for the host) meets every G16 chain
fixture and every G18 edge chain under the bound of tests/_grad_cases.py; the solver's update rule
(env_build_amd/mpc.py, device-agnostic torch) does what it promises on a problem with a known answer; the MPC fixtures
(scripts/gen_golden_mpc.py) are self-consistent."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from tests._helpers import ROOT, HostModel, build_host_harness, golden, oracle_lib, _p
from tests._grad_cases import TASKS, MAX_EXCLUDED, cases, chain_and_edge_cases, check_columns

HEADER = os.path.join(ROOT, 'include', 'envbuild_grad.h')
NEW = ('eb_rollout_tape_vjp', 'eb_rollout_tape_vjp_max_horizon')


def test_header_declares_the_tape_entries_as_ctypes_binds_them():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert name in _capi.GRAD_PROTOTYPES and name not in _capi.PROTOTYPES
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/envbuild_grad.h' % name
        assert len(m.group(1).split(',')) == len(_capi.GRAD_PROTOTYPES[name][1]), name
    assert _capi.EB_GRAD_ABI_VERSION == 2 and _capi.EB_ABI_VERSION == 5
    assert int(re.search(r'#define EB_GRAD_ABI_VERSION (\d+)', src).group(1)) == 2
    # the header no longer says the tape has no reverse pass
    assert 'tape kernels' not in open(HEADER).read()


def test_hip_library_exports_the_tape_entries_and_a_gfx950_kernel():
    lib_path = eb_build.build()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.eb_grad_abi_version() == 2
    blob = open(lib_path, 'rb').read()
    assert b'gfx950' in blob and b'rollout_tape_vjp_kernel' in blob
    assert 'eb_rollout_tape_vjp.hip' in eb_build.SOURCES and 'eb_tape_grad_device.h' in eb_build.HEADERS
    # a translation unit of its own: the forward kernels' hashes (profiles/ ties HBM-traffic records to them) do not see it
    for files in eb_build.KERNEL_SOURCES.values():
        assert 'eb_rollout_tape_vjp.hip' not in files and 'eb_tape_grad_device.h' not in files


def test_a_library_without_the_tape_entries_is_refused_cleanly():
    api = oracle_lib()
    assert api.backend == 'oracle'
    for name in ('rollout_tape_vjp', 'rollout_tape_vjp_max_horizon'):
        with pytest.raises(_capi.EbError) as e:
            getattr(api, name)
        assert 'reverse pass' in str(e.value)
    with pytest.raises(_capi.EbError):
        api.grad_fn('eb_rollout_tape_vjp')


@pytest.fixture(scope='module')
def host_harness(tmp_path_factory):
    """tests/_tape_grad_host_harness.hip: the kernel's __host__ __device__ reverse sweep compiled for the host"""
    return build_host_harness(tmp_path_factory, '_tape_grad_host_harness.hip', 'tape_grad_host')


def oracle_forward(task, c):
    """the pre-step obs of every step [H, B, D] and out5 [H, 5, B] from the CPU oracle (bit-identical to the HIP forward)"""
    m = HostModel(oracle_lib(), task, n_veh=c.n_veh, n_future=c.n_future, mode=c.mode)
    obs, pre, out5 = c['obs0'], [], []
    for a in c['tape']:
        pre.append(obs)
        obs, o5, _ = m.rollout_step(obs, a, c.ref_idx(), c.path_id)
        out5.append(o5)
    return np.ascontiguousarray(np.stack(pre), np.float32), np.stack(out5)


def host_tape_vjp(h, task, c, pre, g_final, g5, w5=None):
    H, n, D = pre.shape
    ri = c['ref_idx']
    has_path = np.ascontiguousarray(((ri >= 0) & (ri < 3)) if c.mode == 'training' else np.ones(n, bool), dtype=np.int32)
    tape = np.ascontiguousarray(c['tape'], np.float32)
    go, ga = np.full((n, c.nd), np.nan, np.float32), np.full((H, n, 2), np.nan, np.float32)
    g5 = None if g5 is None else np.ascontiguousarray(g5, np.float32)
    w5 = None if w5 is None else np.ascontiguousarray(w5, np.float32)
    h.host_tape_vjp(_capi.TASK_ID[task], n, H, D, c.nd, c.n_veh, c.n_future, _p(pre), _p(tape), _p(has_path),
                    _p(np.ascontiguousarray(g_final, np.float32)), _p(g5), _p(w5), _p(go), _p(ga))
    return go, ga


@pytest.mark.parametrize('task', TASKS)
def test_tape_reverse_sweep_on_the_host_meets_the_chain_fixtures(task, host_harness):
    """every G16 case and every chain of G18: |g - g64| <= 4 E_c + 2^-20 max|g64| per column (tests/_grad_cases.py), at most 1 % of
    the rows excluded"""
    cs = chain_and_edge_cases(task)
    rows = excluded = 0
    for c in cs:
        pre, out5 = oracle_forward(task, c)
        want = c['out5_f32'].astype(np.float64)
        ok = c['ok'] & (np.abs(out5 - want) <= 5e-6 + 1e-5 * np.abs(want)).all((0, 1))
        rows += len(ok); excluded += int((~ok).sum())
        go, ga = host_tape_vjp(host_harness, task, c, pre, c['g_obs_final'], c['g_out5_steps'])
        check_columns(go, c['g_obs64'], c['E_obs'], ok, 'host tape %s %s obs0' % (task, c.name))
        check_columns(np.moveaxis(ga, 0, 1), np.moveaxis(c['g_act64'], 0, 1), c['E_act'], ok, 'host tape %s %s tape' % (task, c.name))
    print('host tape %s: %d of %d rows excluded' % (task, excluded, rows))
    assert excluded <= MAX_EXCLUDED * rows


def test_w5_form_equals_a_filled_cotangent_array_on_the_host(host_harness):
    c = cases('g16_grad_chain', 'left')[0]
    pre, _ = oracle_forward('left', c)
    H, n = pre.shape[:2]
    w5 = np.array([-1.0, 10.0, 0.5, 0.25, 2.0], np.float32)
    a = host_tape_vjp(host_harness, 'left', c, pre, c['g_obs_final'], None, w5)
    b = host_tape_vjp(host_harness, 'left', c, pre, c['g_obs_final'], np.broadcast_to(w5[None, :, None], (H, 5, n)))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.abs(a[1]).max() > 0


# ---- the solver's update rule, on the CPU ----
def test_cost_from_out5_is_the_weighted_sum():
    import torch
    from env_build_amd.mpc import cost_from_out5, DEFAULT_WEIGHTS
    assert DEFAULT_WEIGHTS == (-1.0, 10.0, 0.0, 0.0, 0.0)
    o = torch.arange(3 * 5 * 4, dtype=torch.float64).reshape(3, 5, 4)
    assert torch.equal(cost_from_out5(o), (-o[:, 0] + 10.0 * o[:, 1]).sum(0))
    assert torch.equal(cost_from_out5(o, (0, 0, 2, 0, 1)), (2.0 * o[:, 2] + o[:, 4]).sum(0))
    o[1, 3, 2] = float('nan')                       # a row with weight 0 does not enter
    assert torch.isfinite(cost_from_out5(o)).all()
    assert torch.equal(cost_from_out5(o, (0, 0, 0, 0, 0)), torch.zeros(4, dtype=torch.float64))


def test_projected_gradient_solves_box_constrained_quadratics_per_env():
    """J_b(u) = 1/2 sum_i c_i (u_i - m_bi)^2 is separable: its minimiser over the box is clip(m_b).  Every env converges with a
    step length of its own, J never increases, and an env whose cost is NaN keeps its iterate."""
    import torch
    from env_build_amd.mpc import projected_gradient
    g = torch.Generator().manual_seed(0)
    H, B = 25, 7
    m = torch.randn((H, B, 2), generator=g, dtype=torch.float64) * 1.5
    c = torch.rand((H, 1, 2), generator=g, dtype=torch.float64) * 20.0 + 0.05
    scale = torch.tensor([1.0, 1e-3, 50.0, 1.0, 7.0, 0.2, 1.0], dtype=torch.float64)     # envs of very different curvature
    calls = []

    def evaluate(u, need_grad):
        calls.append(need_grad)
        J = (0.5 * c * (u - m) ** 2).sum((0, 2)) * scale
        J[6] = float('nan') if len(calls) > 1 else J[6]                # env 6: every trial is rejected
        return J, (c * (u - m) * scale.view(1, -1, 1) if need_grad else None)
    u, J, info = projected_gradient(evaluate, torch.zeros((H, B, 2), dtype=torch.float64), 200)
    want = m.clamp(-1, 1)
    assert (u.abs() <= 1).all()
    assert (u[:, :6] - want[:, :6]).abs().max() < 1e-6
    assert not u[:, 6].any() and not info['accepted'][:, 6].any()         # kept where it was
    hist = info['J_history'][:, :6]
    assert (hist[1:] <= hist[:-1]).all() and torch.equal(hist[-1], J[:6])
    assert info['launches_per_iteration'] == 4 and info['evaluations'] == 1 + 200 * 4
    assert calls[0] is True and calls[1:5] == [False, False, False, True]  # trials are value-only


def test_warm_start_shifts_the_tape_by_one_step():
    import torch
    from env_build_amd.mpc import OpenLoopMPC
    u = torch.arange(4 * 3 * 2, dtype=torch.float32).reshape(4, 3, 2)
    w = OpenLoopMPC.warm_start(u)
    assert torch.equal(w[:3], u[1:]) and torch.equal(w[3], u[3]) and w.is_contiguous()


@pytest.mark.parametrize('task', TASKS)
def test_mpc_fixtures_are_self_consistent(task):
    z = golden('g17_mpc_%s' % task)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g17_mpc_%s.npz' % task)) <= 64 * 1024
    rows, B = z['rows'], len(z['rows'])
    g5 = golden('g5_rollout_%s_N%d_training_nf0' % (task, {'left': 8, 'straight': 9, 'right': 5}[task]))
    assert 4 <= B <= 16 and len(set(rows.tolist())) == B and rows.max() < len(g5['obs0'])
    assert int(z['horizon']) == 25 and z['u_ref'].shape == (25, B, 2) and np.abs(z['u_ref']).max() <= 1.0
    assert np.array_equal(z['weights'], np.array([-1, 10, 0, 0, 0], np.float32))
    assert z['J0'].dtype == np.float64 and (z['J_ref'] <= z['J0']).all() and np.isfinite(z['J_ref2']).all()
    assert np.array_equal(z['ref_alone_ok'], z['J_ref2'] <= z['J_ref'] + 0.1)
    # the condition on the inputs: the reference ALONE disagrees with itself on at most one quarter of the file's rows
    assert 4 * int((~z['ref_alone_ok']).sum()) <= B


def test_generator_reproduces_the_committed_mpc_fixtures():
    from oracle import refload
    if not refload.available():
        pytest.skip('reference tree not present (build container only)')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'gen_golden_mpc.py'), '--check'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('reproduced') == 3
