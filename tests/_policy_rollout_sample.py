"""What is specific to eb_policy_rollout_sample (include/envbuild_policy_rollout_sample.h) on top of tests/_policy.py and
tests/_policy_rollout_grad.py: the entry as one call through the module's own binding, and the yardstick — the loop of existing single
calls (eb_policy_sample, eb_rollout_step, eb_rollout_step_vjp, eb_policy_sample_vjp, eb_mlp_backward with head 0) through the same two
handles, forward and back.  A helper module like _tape.py and _policy.py: pytest does not collect it, and importing it touches no
device."""
import ctypes as C

import numpy as np

from env_build_amd import policy_rollout as PR, policy_sample as PS
from env_build_amd.policy_sample import policy_noise_reference
from tests import _policy, _policy_rollout_grad as G
from tests._policy import SENTINEL, assert_equal, param_count, same, scene, split_params  # noqa: F401  (its tests reach them through here)
from tests._policy_rollout_grad import W5, model, rows_of as _rows_of  # noqa: F401
from tests._tape import cost_in_the_headers_order

OUTPUTS = ('last', 'out5', 'actions', 'obs', 'cost', 'logp', 'eps', 'g_actions', 'g_obs0', 'g_params')
FORWARD = ('last', 'out5', 'actions', 'obs', 'cost', 'logp', 'eps')
PER_ROW = FORWARD + ('g_actions', 'g_obs0')
GRADS = ('g_actions', 'g_obs0', 'g_params')
FIELD = {'last': 'obs_out', 'out5': 'out5_steps', 'actions': 'actions_steps', 'obs': 'obs_steps', 'cost': 'cost', 'logp': 'logp_steps',
         'eps': 'eps_out_steps', 'g_actions': 'g_actions_steps', 'g_obs0': 'g_obs0', 'g_params': 'g_params'}


def fn(dev, name):
    return PR.bind_sample(dev.api)[name]


def supported(dev, m):
    """eb_policy_rollout_sample_supported -> (ok, the reason eb_last_error holds)"""
    ok = C.c_int32(-7)
    dev.api.check(fn(dev, 'eb_policy_rollout_sample_supported')(dev.h, m, C.byref(ok)))
    return ok.value, dev.api.lib.eb_last_error().decode()


def workspace_bytes(dev, m, n, steps, with_grad=1):
    need = C.c_size_t(0)
    dev.api.check(fn(dev, 'eb_policy_rollout_sample_workspace_bytes')(dev.h, m, int(n), int(steps), int(with_grad), C.byref(need)))
    return need.value


def shapes(n, D, steps, count):
    return {'last': (n, D), 'out5': (steps, 5, n), 'actions': (steps, n, 2), 'obs': (steps, n, D), 'cost': (n,), 'logp': (steps, n),
            'eps': (steps, n, 2), 'g_actions': (steps, n, 2), 'g_obs0': (n, 9), 'g_params': (count,)}


def ids_in(dev, row_ids):
    return None if row_ids is None else dev._in(np.asarray(row_ids).astype(np.uint32).view(np.int32), np.int32)


def call(dev, m, **fields):
    """eb_policy_rollout_sample with the struct's fields given by name (pointers as integers or None)"""
    a = PR.sample_args(**fields)
    dev.api.check(fn(dev, 'eb_policy_rollout_sample')(dev.h, m, C.byref(a)))


def raw(t):
    return None if t is None else t.data_ptr()


def entry(dev, m, obs, steps, w5=W5, w_logp=0.0, ref_idx=None, path_id=0, ar=1.0, eps=None, seed=0, counter=0, row_ids=None, want=OUTPUTS,
          stream=None, ws_fill=None):
    """eb_policy_rollout_sample -> dict of NumPy arrays; an output that is not in `want` is passed as NULL, the others start as SENTINEL.
    Forward-only calls pass no workspace unless ws_fill is given: then a workspace of the with_grad size filled with it, returned as 'ws'"""
    torch = dev.torch
    ob, ri, ep, ids = dev._in(obs), dev._in(ref_idx, np.int32), dev._in(eps), ids_in(dev, row_ids)
    n, D = ob.shape
    with_grad = any(k in want for k in GRADS)
    need = workspace_bytes(dev, m, n, steps, with_grad)
    ws = None
    if need or ws_fill is not None:
        ws = torch.full((max(workspace_bytes(dev, m, n, steps, 1), 16) // 4,), SENTINEL if ws_fill is None else ws_fill, device=dev.dev)
    bufs = {k: (torch.full(s, SENTINEL, device=dev.dev) if k in want else None) for k, s in shapes(n, D, steps, param_count(dev, m)).items()}
    call(dev, m, n_env=n, steps=int(steps), path_id=int(path_id), action_range=float(ar), w_logp=float(w_logp), w5=w5, seed=int(seed),
         counter=int(counter), obs_in=raw(ob), ref_idx=raw(ri), row_ids=raw(ids), eps_steps=raw(ep), workspace=raw(ws),
         workspace_bytes=0 if ws is None else ws.numel() * 4, stream=dev.stream if stream is None else stream,
         **{FIELD[k]: raw(v) for k, v in bufs.items()})
    out = {k: dev._ret(v) for k, v in bufs.items() if v is not None}
    if ws_fill is not None:
        out['ws'] = dev._ret(ws)
    return out


def mlp_backward0(dev, m, obs, g, want_params):
    """one eb_mlp_backward with head 0 over device tensors -> (g_obs or None, g_params or None) as device tensors"""
    torch = dev.torch
    n = obs.shape[0]
    need = C.c_size_t(0)
    dev.api.mlp_backward_workspace_bytes(m, n, C.byref(need))
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev.dev)
    g_obs = None if want_params else torch.empty_like(obs)
    g_par = torch.empty((param_count(dev, m),), device=dev.dev) if want_params else None
    p = dev._ptr
    dev.api.mlp_backward(m, n, p(obs), p(g), 0, C.c_float(0.0), p(ws), need.value, None, p(g_obs), p(g_par), dev.stream)
    return g_obs, g_par


def loop(dev, m, obs0, steps, w5=W5, w_logp=0.0, ref_idx=None, path_id=0, ar=1.0, eps=None, seed=0, counter=0, row_ids=None, grad=True,
         g_params=False):
    """the yardstick the header states: `steps` x [eb_policy_sample(seed, counter + t) -> eb_rollout_step], then for t = steps - 1 .. 0
    eb_rollout_step_vjp with g_obs_out = lambda_{t+1} and g_out5 = w5 at every env, eb_policy_sample_vjp with g_logp = w_logp in every
    row, eb_mlp_backward (head 0) on its g_logits, lambda_t = s_t[:, :9] + p_t[:, :9].  With g_params, one more eb_mlp_backward over the
    steps * n rows (t, env) in t-major order.  Also 'pre' (obs_t), 'y' (the logits) and 'g_y'.  `dev` is a TapeModel."""
    torch = dev.torch
    sample = PS.bind(dev.api)
    ob, ri, ep, ids = dev._in(obs0), dev._in(ref_idx, np.int32), dev._in(eps), ids_in(dev, row_ids)
    n, D = ob.shape
    new = lambda *s: torch.empty(s, device=dev.dev)
    pre, acts, out5s, logps, used, ys = [ob], [], [], [], [], []
    sc = new(n, 2)
    p = dev._ptr
    for t in range(steps):
        a, lp, y, e, nxt, o5 = new(n, 2), new(n), new(n, 4), new(n, 2), new(n, D), new(5, n)
        dev.api.check(sample['eb_policy_sample'](m, n, raw(pre[t]), None if ep is None else raw(ep[t]), raw(ids), int(seed), int(counter) + t,
                                                 float(ar), raw(a), raw(lp), raw(y), raw(e), dev.stream))
        dev.api.rollout_step(dev.h, n, p(pre[t]), p(a), p(ri), int(path_id), p(nxt), p(o5), p(sc), dev.stream)
        pre.append(nxt); acts.append(a); out5s.append(o5); logps.append(lp); used.append(e); ys.append(y)
    out5 = torch.stack(out5s)
    ret = lambda v: dev._ret(v.contiguous())
    out = {'last': ret(pre[steps]), 'out5': ret(out5), 'actions': ret(torch.stack(acts)), 'obs': ret(torch.stack(pre[1:])),
           'cost': cost_in_the_headers_order(out5[None], w5)[0], 'logp': ret(torch.stack(logps)), 'eps': ret(torch.stack(used)),
           'pre': ret(torch.stack(pre[:steps])), 'y': ret(torch.stack(ys))}
    if not grad:
        return out
    lam = torch.zeros((n, 9), device=dev.dev)
    g5 = torch.tensor([float(v) for v in w5], device=dev.dev).view(5, 1).expand(5, n).contiguous()
    g_lp = torch.full((n,), float(w_logp), device=dev.dev)
    gas, gys = [None] * steps, [None] * steps
    for t in range(steps - 1, -1, -1):
        s, ga = dev.t_step_vjp(pre[t], acts[t], ri, path_id, lam, g5)
        gy = new(n, 4)
        dev.api.check(sample['eb_policy_sample_vjp'](n, 4, raw(ys[t]), raw(used[t]), float(ar), raw(ga), raw(g_lp), raw(gy), dev.stream))
        pt, _ = mlp_backward0(dev, m, pre[t], gy, False)
        lam = (s[:, :9] + pt[:, :9]).contiguous()
        gas[t], gys[t] = ga, gy
    out.update({'g_actions': ret(torch.stack(gas)), 'g_obs0': ret(lam), 'g_y': ret(torch.stack(gys))})
    if g_params:
        rows, g = torch.cat(pre[:steps]).contiguous(), torch.cat(gys).contiguous()
        out['g_params'] = ret(mlp_backward0(dev, m, rows, g, True)[1])
    return out


def rows_of(d, idx):
    """the per-row outputs of `d` for the envs idx"""
    pick = {'last': lambda v: v[idx], 'cost': lambda v: v[idx], 'g_obs0': lambda v: v[idx], 'out5': lambda v: v[:, :, idx]}
    return {k: pick.get(k, lambda v: v[:, idx])(v) for k, v in d.items() if k in PER_ROW}


SEED = 0x5EED


def given_noise(steps, B, seed=3):
    return np.random.default_rng(seed).standard_normal((steps, B, 2)).astype(np.float32)


def forward_equals_the_loop(case, sizes=(1, 63, 64, 65, 200), horizons=(1, 5), long=25, others=True):
    """case = (task, N, units, hidden layers, hidden activation): every forward output of the entry equals the loop's bit for bit, noise
    drawn and given (tests/test_gpu_policy_rollout_sample.py and the rows of tests/test_gpu_kernel_census.py call this one text); at 200
    rows also `long` steps, with the loop's own premise; `others`: the other heads, no scale, selecting mode, a counter, row ids."""
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = scene(task, N, units, n_hidden, hact=hact)
    dev = model(task, N)
    m = dev.make_mlp(*net, scale)
    assert supported(dev, m)[0] == 1
    for B in sizes:
        for steps in tuple(horizons) + ((long,) if B == 200 else ()):
            for eps in (None, given_noise(steps, B)):
                kw = dict(ref_idx=ref_idx[:B], eps=eps, seed=SEED)
                ref = loop(dev, m, obs0[:B], steps, W5, grad=False, **kw)
                what = '%s B=%d steps=%d noise %s' % (case, B, steps, 'drawn' if eps is None else 'given')
                assert_equal(entry(dev, m, obs0[:B], steps, W5, want=FORWARD, **kw), ref, what, FORWARD)
                if eps is None:
                    for t in range(steps):
                        assert same(ref['eps'][t], policy_noise_reference(np.arange(B), 2, SEED, t)), what
                else:
                    assert same(ref['eps'], eps)
            if B == 200 and steps == long:         # the LOOP's own outputs (noise drawn) reach what the kernel has to get right
                ref = loop(dev, m, obs0, steps, W5, ref_idx=ref_idx, seed=SEED, grad=False)
                hit, road = (ref['out5'][:, 3] > 0).any(0), (ref['out5'][:, 4] > 0).any(0)
                x = np.abs(ref['y'][:, :, :2].astype(np.float64) + np.exp(ref['y'][:, :, 2:].astype(np.float64)) * ref['eps'])
                assert hit.any() and (~hit).any() and road.any() and (~road).any() and np.all(np.isfinite(ref['obs']))
                assert (x < 0.6).any() and (x > 0.65).any()            # both branches of the deterministic tanh (0.625)
                print('%s N=%d: %d rows collide, %d hit a wall, %.0f%% of |x| below 0.625' % (task, N, int(hit.sum()), int(road.sum()),
                                                                                           100.0 * (x < 0.625).mean()))
    if others:
        B = 200
        sel = model(task, N, 'selecting')
        m_plain = dev.make_mlp(*net)
        assert supported(sel, m_plain)[0] == 1
        ids = np.random.default_rng(9).integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
        for mm, mdl, kw in ((m, dev, dict(ref_idx=ref_idx, ar=0.5)), (m, dev, dict(ref_idx=ref_idx, ar=-1.0)),
                            (m_plain, dev, dict(ref_idx=ref_idx)), (m, sel, dict(path_id=0)), (m_plain, sel, dict(path_id=2)),
                            (m, dev, dict(ref_idx=ref_idx, counter=2 ** 40 + 7)), (m, dev, dict(ref_idx=ref_idx, row_ids=ids))):
            ref = loop(mdl, mm, obs0, 5, W5, seed=SEED, grad=False, **kw)
            assert np.all(np.isfinite(ref['obs']))
            assert_equal(entry(mdl, mm, obs0, 5, W5, seed=SEED, want=FORWARD, **kw), ref, '%s %s' % (case, sorted(kw)), FORWARD)
            if 'row_ids' in kw:
                assert same(ref['eps'][3], policy_noise_reference(ids, 2, SEED, 3))
            if 'counter' in kw:
                assert same(ref['eps'][4], policy_noise_reference(np.arange(B), 2, SEED, 2 ** 40 + 11))
        dev.api.mlp_destroy(m_plain)
    dev.api.mlp_destroy(m)


def reverse_equals_the_loop(case, sizes=(1, 65, 200), horizons=(1, 5)):
    """every per-row output, gradients included, equals the loop's bit for bit over four (w_logp, action_range, noise) combinations;
    w_logp = 0 and eps = 0 against eb_policy_rollout_grad"""
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = scene(task, N, units, n_hidden, hact=hact)
    dev = model(task, N)
    m = dev.make_mlp(*net, scale)
    for B in sizes:
        for steps in horizons:
            w5 = tuple(v / (steps * B) for v in W5)
            for w_logp, ar, eps in ((0.0, 1.0, None), (0.3, 1.0, None), (0.3, 0.5, given_noise(steps, B)), (0.3, -1.0, None)):
                kw = dict(w_logp=w_logp, ref_idx=ref_idx[:B], ar=ar, eps=eps, seed=SEED, counter=5)
                ref = loop(dev, m, obs0[:B], steps, w5, **kw)
                got = entry(dev, m, obs0[:B], steps, w5, **kw)
                assert_equal(got, ref, '%s B=%d steps=%d w_logp %g ar %g' % (case, B, steps, w_logp, ar), PER_ROW)
                assert (B == 1 or np.any(ref['g_actions'] != 0)) and np.all(np.isfinite(ref['g_obs0']))   # (one row may sit beyond the clip)
                only = entry(dev, m, obs0[:B], steps, w5, want=('g_obs0',), **kw)
                assert sorted(only) == ['g_obs0'] and same(only['g_obs0'], ref['g_obs0'])
            # w_logp = 0 and eps = 0 against eb_policy_rollout_grad.  With action_range = 1 the identity holds on EVERY column of
            # g_actions and g_obs0, as numbers: the head's cotangent g * (1 * (1 - t^2)) + 0 * 2t is the parent's (g * 1) * (1 - t^2),
            # and the log-std columns' s * (std * 0) - 0 are zeros, which add nothing to the products with W^T (a zero's sign may
            # differ, hence == and not the bits).  With another action_range the two roundings of g * ar * (1 - t^2) differ, and only
            # the LAST step's g_actions — the model step's reverse from lambda = 0, no policy in it — is asserted.
            zero = np.zeros((steps, B, 2), np.float32)
            for ar in (1.0, 0.5):
                det = G.entry(dev, m, obs0[:B], steps, w5, ref_idx[:B], ar=ar, want=('g_actions', 'g_obs0'))
                got = entry(dev, m, obs0[:B], steps, w5, w_logp=0.0, ref_idx=ref_idx[:B], ar=ar, eps=zero, want=('g_actions', 'g_obs0'))
                assert np.array_equal(got['g_actions'][-1], det['g_actions'][-1])
                if ar == 1.0:
                    assert np.array_equal(got['g_actions'], det['g_actions']) and np.array_equal(got['g_obs0'], det['g_obs0'])
    dev.api.mlp_destroy(m)
