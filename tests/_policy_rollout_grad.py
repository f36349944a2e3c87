"""What is specific to eb_policy_rollout_grad (include/envbuild_policy_rollout_grad.h) on top of tests/_policy.py: the entry as one call,
and the yardstick — the loop of existing single calls through the same two handles, forward and back.  A helper module like _tape.py
and _policy.py: pytest does not collect it, and importing it touches no device."""
import ctypes as C
import functools

import numpy as np

from tests import _policy
from tests._policy import SENTINEL, assert_equal, param_count, same, scene, split_params  # noqa: F401  (its tests reach them through here)
from tests._tape import TapeModel, cost_in_the_headers_order

W5 = (-1.0, 10.0, 0.0, 0.0, 0.0)                # ADP's loss before its 1 / (steps * n_env): rewards against the training penalty
OUTPUTS = ('last', 'out5', 'actions', 'obs', 'cost', 'g_actions', 'g_obs0', 'g_params')
PER_ROW = ('last', 'out5', 'actions', 'obs', 'cost', 'g_actions', 'g_obs0')
supported = functools.partial(_policy.supported, family='policy_rollout_grad')


def floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def workspace_bytes(dev, m, n, steps):
    need = C.c_size_t(0)
    dev.api.policy_rollout_grad_workspace_bytes(dev.h, m, int(n), int(steps), C.byref(need))
    return need.value


def shapes(n, D, steps, count):
    return {'last': (n, D), 'out5': (steps, 5, n), 'actions': (steps, n, 2), 'obs': (steps, n, D), 'cost': (n,),
            'g_actions': (steps, n, 2), 'g_obs0': (n, 9), 'g_params': (count,)}


def entry(dev, m, obs, steps, w5=W5, ref_idx=None, path_id=0, ar=1.0, want=OUTPUTS):
    """eb_policy_rollout_grad -> dict of NumPy arrays; an output that is not in `want` is passed as NULL, the others start as SENTINEL"""
    torch = dev.torch
    ob, ri = dev._in(obs), dev._in(ref_idx, np.int32)
    n, D = ob.shape
    need = workspace_bytes(dev, m, n, steps)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev.dev)
    bufs = {k: (torch.full(s, SENTINEL, device=dev.dev) if k in want else None) for k, s in shapes(n, D, steps, param_count(dev, m)).items()}
    p = dev._ptr
    dev.api.policy_rollout_grad(dev.h, m, n, int(steps), p(ob), p(ri), int(path_id), C.c_float(ar), floats(w5), p(ws), need,
                                *[p(bufs[k]) for k in OUTPUTS], dev.stream)
    return {k: dev._ret(v) for k, v in bufs.items() if v is not None}


def mlp_backward(dev, m, obs, g, ar, want_params):
    """one eb_mlp_backward with head 1 over device tensors -> (g_obs or None, g_params or None) as device tensors"""
    torch = dev.torch
    n = obs.shape[0]
    need = C.c_size_t(0)
    dev.api.mlp_backward_workspace_bytes(m, n, C.byref(need))
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev.dev)
    g_obs = None if want_params else torch.empty_like(obs)
    g_par = torch.empty((param_count(dev, m),), device=dev.dev) if want_params else None
    p = dev._ptr
    dev.api.mlp_backward(m, n, p(obs), p(g), 1, C.c_float(ar), p(ws), need.value, None, p(g_obs), p(g_par), dev.stream)
    return g_obs, g_par


def loop(dev, m, obs0, steps, w5=W5, ref_idx=None, path_id=0, ar=1.0, g_params=False):
    """the yardstick: `steps` x [eb_policy_run_batch -> eb_rollout_step], then for t = steps - 1 .. 0 eb_rollout_step_vjp with
    g_obs_out = lambda_{t+1} and g_out5 = w5 at every env, eb_mlp_backward (head 1) on its g_actions, lambda_t = s_t[:, :9] + p_t[:, :9].
    With g_params, one more eb_mlp_backward over the steps * n rows (t, env) in t-major order.  `dev` is a TapeModel."""
    torch = dev.torch
    ob, ri = dev._in(obs0), dev._in(ref_idx, np.int32)
    n, D = ob.shape
    pre, acts, out5s = [ob], [], []
    sc = torch.empty((n, 2), device=dev.dev)
    p = dev._ptr
    for t in range(steps):
        a, nxt, o5 = torch.empty((n, 2), device=dev.dev), torch.empty((n, D), device=dev.dev), torch.empty((5, n), device=dev.dev)
        dev.api.policy_run_batch(m, n, p(pre[t]), C.c_float(ar), p(a), dev.stream)
        dev.api.rollout_step(dev.h, n, p(pre[t]), p(a), p(ri), int(path_id), p(nxt), p(o5), p(sc), dev.stream)
        pre.append(nxt); acts.append(a); out5s.append(o5)
    lam = torch.zeros((n, 9), device=dev.dev)
    g5 = torch.tensor([float(v) for v in w5], device=dev.dev).view(5, 1).expand(5, n).contiguous()
    gas = [None] * steps
    for t in range(steps - 1, -1, -1):
        s, ga = dev.t_step_vjp(pre[t], acts[t], ri, path_id, lam, g5)
        pt, _ = mlp_backward(dev, m, pre[t], ga, ar, False)
        lam = (s[:, :9] + pt[:, :9]).contiguous()
        gas[t] = ga
    out5 = torch.stack(out5s)
    ret = lambda v: dev._ret(v.contiguous())
    out = {'last': ret(pre[steps]), 'out5': ret(out5), 'actions': ret(torch.stack(acts)), 'obs': ret(torch.stack(pre[1:])),
           'cost': cost_in_the_headers_order(out5[None], w5)[0], 'g_actions': ret(torch.stack(gas)), 'g_obs0': ret(lam),
           'pre': ret(torch.stack(pre[:steps]))}
    if g_params:
        rows, g = torch.cat(pre[:steps]).contiguous(), torch.cat(gas).contiguous()
        out['g_params'] = ret(mlp_backward(dev, m, rows, g, ar, True)[1])
    return out


def rows_of(d, idx):
    """the per-row outputs of `d` for the envs idx"""
    pick = {'last': lambda v: v[idx], 'cost': lambda v: v[idx], 'g_obs0': lambda v: v[idx], 'out5': lambda v: v[:, :, idx]}
    return {k: pick.get(k, lambda v: v[:, idx])(v) for k, v in d.items() if k in PER_ROW}


def model(task, N, mode='training'):
    return TapeModel(task, n_veh=N, mode=mode)


PREMISE = {('left', 8), ('right', 5), ('straight', 32)}


def forward_and_reverse_equal_the_loop(case, sizes=(1, 63, 64, 65, 200), horizons=(1, 5, 25), only_g_params_at=5, others=True):
    """case = (task, N, units, hidden layers, hidden activation): every per-row output of the entry equals the loop's bit for bit at
    every batch size and horizon (tests/test_gpu_policy_rollout_grad.py and the rows of tests/test_gpu_kernel_census.py call this one
    text); `others`: the other heads (with the output weights scaled up: raw actions beyond the clip, a blocked cotangent), no scale,
    selecting mode — at 200 rows, 5 steps."""
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = scene(task, N, units, n_hidden, hact=hact)
    dev = model(task, N)
    m = dev.make_mlp(*net, scale)
    assert supported(dev, m)[0] == 1
    w5 = tuple(v / (25 * 200) for v in W5)
    for B in sizes:
        for steps in horizons:
            ref = loop(dev, m, obs0[:B], steps, w5, ref_idx[:B])
            what = '%s B=%d steps=%d' % (case, B, steps)
            assert_equal(entry(dev, m, obs0[:B], steps, w5, ref_idx[:B]), ref, what, PER_ROW)
            if steps == only_g_params_at:
                only = entry(dev, m, obs0[:B], steps, w5, ref_idx[:B], want=('g_params',))
                assert sorted(only) == ['g_params'] and np.all(np.isfinite(only['g_params'])) and np.any(only['g_params'] != 0)
            if B == 200 and steps == 25 and (task, N) in PREMISE:          # the loop's own outputs reach what the kernel has to get right
                hit, road = (ref['out5'][:, 3] > 0).any(0), (ref['out5'][:, 4] > 0).any(0)
                assert hit.any() and (~hit).any() and road.any() and np.all(np.isfinite(ref['obs']))
                moved = (ref['g_actions'] != 0).any((0, 2))
                assert moved.mean() > 0.5 and np.any(ref['g_obs0'] != 0)
                print('%s N=%d: %d rows collide, %d hit a wall, %d of %d rows with a non-zero g_actions' % (
                    task, N, int(hit.sum()), int(road.sum()), int(moved.sum()), B))
    if others:
        sel = model(task, N, 'selecting')
        m_plain = dev.make_mlp(*net)
        assert supported(sel, m_plain)[0] == 1
        big = scene(task, N, units, n_hidden, hact=hact, gain=40.0)[2]
        m_big = dev.make_mlp(*big, scale)
        for mm, ar in ((m, 0.5), (m_big, -1.0)):
            ref = loop(dev, mm, obs0, 5, W5, ref_idx, ar=ar)
            if ar < 0:
                beyond = np.abs(ref['actions']) > 1.05
                assert beyond.any() and (~beyond).any() and np.all(ref['g_actions'][beyond] == 0) and np.all(np.isfinite(ref['obs']))
            assert_equal(entry(dev, mm, obs0, 5, W5, ref_idx, ar=ar), ref, '%s action_range %g' % (case, ar), PER_ROW)
        ref = loop(dev, m_plain, obs0, 5, W5, ref_idx)
        assert_equal(entry(dev, m_plain, obs0, 5, W5, ref_idx), ref, '%s no scale' % (case,), PER_ROW)
        for path_id in (0, 2):
            for mm in (m, m_plain):
                ref = loop(sel, mm, obs0, 5, W5, None, path_id)
                assert_equal(entry(sel, mm, obs0, 5, W5, None, path_id), ref, '%s selecting path %d' % (case, path_id), PER_ROW)
        for mm in (m_plain, m_big):
            dev.api.mlp_destroy(mm)
    dev.api.mlp_destroy(m)
