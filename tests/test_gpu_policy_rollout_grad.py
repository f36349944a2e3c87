"""GPU (-m gpu): the closed-loop rollout with its parameter gradient (env_build_amd/csrc/eb_policy_rollout_grad.hip,
include/envbuild_policy_rollout_grad.h) through the C-ABI and the façade.  The yardstick everywhere is tests/_policy_rollout_grad.py's
loop of existing single calls through the same two handles: (1) forward and reverse bit for bit, (2) g_params bit for bit at multiples
of 64 envs, (3) g_params within rule (2) of DESIGN §17 at other batch sizes, (4) repeatability and row independence, (5) refusals,
(6) the façade, the autograd loss and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from env_build_amd import _capi  # noqa: E402
from env_build_amd.policy_grad import mlp_backward_reference  # noqa: E402
from tests import _policy, _policy_rollout_grad as H  # noqa: E402
from tests._policy import F16, F32  # noqa: E402
from tests._policy_cases import make_layers  # noqa: E402

pytestmark = pytest.mark.gpu
W5 = H.W5


# ---- 1: forward and reverse == the loop ----
#        task, N, units, hidden layers, hidden activation
CASES = [('left', 8, 256, 2, 'elu'), ('right', 5, 64, 1, 'relu'), ('straight', 32, 256, 2, 'tanh'), ('left', 32, 128, 3, 'relu'),
         ('left', 1, 100, 2, 'elu')]
assert H.PREMISE == {('left', 8), ('right', 5), ('straight', 32)}


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s_N%d_%dx%d_%s' % (c[0], c[1], c[3], c[2], c[4]))
def test_forward_and_reverse_equal_the_loop(case):
    """the body: tests/_policy_rollout_grad.forward_and_reverse_equal_the_loop"""
    H.forward_and_reverse_equal_the_loop(case, sizes=(1, 63, 64, 65, 200), horizons=(1, 5, 25), only_g_params_at=5, others=True)


# ---- 2: g_params bit for bit at multiples of 64 ----
@pytest.mark.parametrize('case', [('left', 8, 256, 2, 'elu'), ('right', 5, 64, 1, 'relu'), ('left', 1, 100, 2, 'tanh')],
                         ids=lambda c: '%s_N%d_%dx%d_%s' % (c[0], c[1], c[3], c[2], c[4]))
def test_g_params_equal_one_backward_over_the_concatenated_rows(case):
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = H.scene(task, N, units, n_hidden, B=1088, hact=hact)
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    for B in (64, 128, 1088):                       # 1088 x 25 rows: 54 row splits, the last of 64 rows
        for steps in (1, 5, 25):
            w5 = tuple(v / (steps * B) for v in W5)
            ref = H.loop(dev, m, obs0[:B], steps, w5, ref_idx[:B], g_params=True)
            got = H.entry(dev, m, obs0[:B], steps, w5, ref_idx[:B])
            H.assert_equal(got, ref, '%s B=%d steps=%d' % (case, B, steps), H.PER_ROW + ('g_params',))
            assert np.any(ref['g_params'] != 0) and np.all(np.isfinite(ref['g_params']))
    dev.api.mlp_destroy(m)


# ---- 3: g_params at other batch sizes, within rule (2) of DESIGN §17 ----
@pytest.mark.parametrize('case', [('left', 8, 256, 2, 'elu', 5), ('straight', 32, 128, 3, 'tanh', 5), ('right', 5, 64, 1, 'elu', 25)],
                         ids=lambda c: '%s_N%d_%dx%d_%s_%dsteps' % c)
def test_g_params_within_the_bound_at_ragged_batch_sizes(case):
    """per tensor |g_params - ref64| <= 4 E + 2^-20 max |ref64|: ref64 = mlp_backward_reference(float64) over the concatenated rows with
    the kernel's own obs_t and g_a_t, E the float32 restatement's distance from it.  Measured worst error / tolerance: DESIGN §18."""
    task, N, units, n_hidden, hact, steps = case
    obs0, ref_idx, net, scale = H.scene(task, N, units, n_hidden, hact=hact)
    dims, layers = net[:4], net[6]
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    worst, failures = 0.0, []
    for B in (1, 63, 65, 200):
        w5 = tuple(v / (steps * B) for v in W5)
        got = H.entry(dev, m, obs0[:B], steps, w5, ref_idx[:B])
        pre = np.concatenate([obs0[None, :B], got['obs'][:-1]]).reshape(steps * B, -1)
        g = got['g_actions'].reshape(steps * B, 2)
        r32 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 1, 1.0, dtype=np.float32)[2]
        r64 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 1, 1.0, dtype=np.float64)[2]
        for k, (a, b32, b64) in enumerate(zip(H.split_params(got['g_params'], dims), r32, r64)):
            tol = 4.0 * np.abs(b32.astype(np.float64) - b64).max() + 2.0 ** -20 * np.abs(b64).max()
            ratio = float(np.abs(a.astype(np.float64) - b64).max() / max(tol, 1e-300))
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                failures.append((B, k, ratio))
        assert np.any(got['g_params'] != 0)
    print('%s: worst error / tolerance %.3f' % (case, worst))
    assert not failures, failures
    dev.api.mlp_destroy(m)


# ---- 4: rows, calls ----
def test_calls_repeat_and_rows_are_independent():
    task, N = 'left', 8
    obs0, ref_idx, net, scale = H.scene(task, N, 256, 2)
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    first = H.entry(dev, m, obs0, 5, W5, ref_idx)
    H.assert_equal(H.entry(dev, m, obs0, 5, W5, ref_idx), first, 'second call')
    perm = np.random.default_rng(5).permutation(len(obs0))
    H.assert_equal(H.rows_of(H.entry(dev, m, obs0[perm], 5, W5, ref_idx[perm]), slice(None)), H.rows_of(first, perm), 'permuted batch')
    sl = np.arange(100, 171)
    H.assert_equal(H.rows_of(H.entry(dev, m, obs0[sl], 5, W5, ref_idx[sl]), slice(None)), H.rows_of(first, sl), 'slice')
    # non-finite values in two rows' egos and two rows' records: the loop's bits in those rows, every other row untouched
    bad = obs0.copy()
    bad[7, 3], bad[70, 4], bad[130, 9 + 4 * 2], bad[131, 9 + 4 * 3 + 3] = np.nan, np.inf, np.nan, -np.inf
    got = H.entry(dev, m, bad, 5, W5, ref_idx)
    H.assert_equal(got, H.loop(dev, m, bad, 5, W5, ref_idx), 'non-finite rows', H.PER_ROW)
    keep = np.setdiff1d(np.arange(len(obs0)), [7, 70, 130, 131])
    H.assert_equal(H.rows_of(got, keep), H.rows_of(first, keep), 'rows next to non-finite ones')
    assert not np.all(np.isfinite(got['last'][[7, 70, 130, 131]]))
    # n_env = 0: zeros to g_params, nothing else
    torch = dev.torch
    count = H.param_count(dev, m)
    g_par, other = torch.full((count,), H.SENTINEL, device=dev.dev), torch.full((64,), H.SENTINEL, device=dev.dev)
    p = dev._ptr
    dev.api.policy_rollout_grad(dev.h, m, 0, 5, None, None, 0, C.c_float(1.0), H.floats(W5), None, 0, p(other), p(other), p(other), p(other),
                                p(other), p(other), p(other), p(g_par), dev.stream)
    assert bool((dev._ret(g_par) == 0).all()) and bool((dev._ret(other) == H.SENTINEL).all())
    dev.api.policy_rollout_grad(dev.h, m, 0, 5, None, None, 0, C.c_float(1.0), None, None, 0, *([None] * 8), dev.stream)
    assert H.workspace_bytes(dev, m, 0, 5) == 0
    dev.api.mlp_destroy(m)


# ---- 5: what the kernel takes, and the refusals ----
def refused(dev, m, obs, match, ref_idx=None, exc=ValueError, **kw):
    """eb_policy_rollout_grad raises with `match` in the message and writes nothing"""
    torch = dev.torch
    ob, ri = dev._in(obs), dev._in(ref_idx, np.int32)
    n, D = ob.shape
    steps = kw.get('steps', 5)
    shp = H.shapes(n, D, min(max(steps, 1), 5), 70000)
    outs = [torch.empty(shp[k], device=dev.dev) for k in H.OUTPUTS]
    ws = torch.empty((kw.get('ws_floats', 1 << 22),), device=dev.dev)
    p = dev._ptr
    _policy.refused(dev, lambda w, *o: dev.api.policy_rollout_grad(dev.h, m, kw.get('n', n), steps, p(ob), p(ri), kw.get('path_id', 0),
                                                                   C.c_float(1.0), H.floats(W5), w, kw.get('ws_bytes', ws.numel() * 4), *o,
                                                                   dev.stream), [ws] + outs, match, exc)


def test_supported_says_what_the_kernel_takes_and_the_entry_refuses_the_rest():
    rng = np.random.default_rng(0)
    dev = H.model('left', 8)
    D = dev.D
    obs = rng.standard_normal((70, D)).astype(np.float32)
    ri = np.zeros(70, np.int32)

    def net(d, units, out, precision=F32):
        m = dev.make_mlp(d, 2, units, out, 'elu', 'linear', make_layers(rng, d, 2, units, out))
        dev.api.mlp_set_precision(m, precision)
        return m
    good = net(D, 256, 4)
    assert H.supported(dev, good)[0] == 1
    cases = [(dev, net(D, 256, 4, F16), 'precision must be EB_MLP_PRECISION_F32'),
             (dev, net(D, 300, 4), 'pads to 512'),
             (dev, net(D + 4, 256, 4), 'obs_dim %d is not the model' % (D + 4)),
             (dev, net(D, 256, 2), 'out_dim 2 is not 4')]
    wide = H.model('left', 64)
    cases.append((wide, net(wide.D, 256, 4), 'n_veh 64 exceeds'))
    fut = H.TapeModel('left', n_veh=8, n_future=1)
    cases.append((fut, net(fut.D, 256, 4), 'n_future 1 is not supported'))
    for model, m, reason in cases:
        ok, why = H.supported(model, m)
        assert ok == 0 and reason in why and 'eb_policy_rollout_grad' in why, (reason, why)
        refused(model, m, rng.standard_normal((70, model.D)).astype(np.float32), reason, ref_idx=ri)
        with pytest.raises(ValueError, match=reason):
            H.workspace_bytes(model, m, 70, 5)
        dev.api.mlp_destroy(m)
    # the remaining bad arguments
    with pytest.raises(ValueError, match='eb_policy_rollout_grad_supported: null handle'):
        dev.api.policy_rollout_grad_supported(None, good, C.byref(C.c_int32()))
    with pytest.raises(ValueError, match='eb_policy_rollout_grad_supported: null policy'):
        dev.api.policy_rollout_grad_supported(dev.h, None, C.byref(C.c_int32()))
    with pytest.raises(ValueError, match='null output pointer'):
        dev.api.policy_rollout_grad_supported(dev.h, good, None)
    refused(dev, None, obs, 'eb_policy_rollout_grad: null policy', ref_idx=ri)
    cap = _capi.POLICY_ROLLOUT_GRAD_MAX_STEPS
    refused(dev, good, obs, 'steps 0 is outside 1 .. %d' % cap, ref_idx=ri, steps=0)
    refused(dev, good, obs, 'steps %d is outside 1 .. %d' % (cap + 1, cap), ref_idx=ri, steps=cap + 1)
    refused(dev, good, obs, 'n_env < 0', ref_idx=ri, n=-1)
    refused(dev, good, obs, 'rows, one row reduction takes', ref_idx=ri, n=2 ** 31 - 64, steps=cap)
    refused(dev, good, obs, 'training mode needs ref_idx')
    need = H.workspace_bytes(dev, good, 70, 5)
    assert need % 4 == 0 and need < (1 << 24)
    refused(dev, good, obs, 'the workspace holds %d bytes' % (need - 4), ref_idx=ri, ws_bytes=need - 4)
    sel = H.model('left', 8, 'selecting')
    refused(sel, good, obs, 'bad path_id', path_id=3)
    refused(sel, good, obs, 'bad path_id', path_id=-1)
    ob, ws = dev._in(obs), dev._out((need // 4,))
    rip, w5 = dev._ptr(dev._in(ri, np.int32)), H.floats(W5)
    none8 = [None] * 8
    for args, match in (((None, rip, 0, C.c_float(1.0), w5, dev._ptr(ws), need), 'null obs_in, w5 or workspace'),
                        ((dev._ptr(ob), rip, 0, C.c_float(1.0), None, dev._ptr(ws), need), 'null obs_in, w5 or workspace'),
                        ((dev._ptr(ob), rip, 0, C.c_float(1.0), w5, None, need), 'null obs_in, w5 or workspace')):
        with pytest.raises(ValueError, match=match):
            dev.api.policy_rollout_grad(dev.h, good, 70, 5, *args, *none8, dev.stream)
    with pytest.raises(ValueError, match='obs_out must not alias obs_in'):
        dev.api.policy_rollout_grad(dev.h, good, 70, 5, dev._ptr(ob), rip, 0, C.c_float(1.0), w5, dev._ptr(ws), need, dev._ptr(ob),
                                    *([None] * 7), dev.stream)
    assert H.same(dev._ret(ob), obs)
    with pytest.raises(ValueError, match='eb_policy_rollout_grad: null handle'):
        dev.api.policy_rollout_grad(None, good, 70, 5, dev._ptr(ob), rip, 0, C.c_float(1.0), w5, dev._ptr(ws), need, *none8, dev.stream)
    # EB_ESTATE: a policy whose layers were never set
    cfg = _capi.EbMlpConfig(_capi.EB_ABI_VERSION, D, 2, 256, 4, _capi.ACT_ID['elu'], _capi.ACT_ID['linear'], 0)
    bare = C.c_void_p()
    dev.api.check(dev.api.lib.eb_mlp_create(C.byref(cfg), C.byref(bare)))
    ok, why = H.supported(dev, bare)
    assert ok == 0 and 'a layer was never set' in why
    refused(dev, bare, obs, 'a layer was never set', ref_idx=ri, exc=_capi.EbError)
    dev.api.mlp_destroy(bare)
    assert dev.api.policy_rollout_grad_fn('eb_policy_rollout_grad_abi_version')() == _capi.EB_POLICY_ROLLOUT_GRAD_ABI_VERSION == 1
    dev.api.mlp_destroy(good)


# ---- 6: façade ----
def rule2(got, layers, pre, g, hact, scale, dims, what):
    """rule (2) of DESIGN §17 per parameter tensor: |got - ref64| <= 4 E + 2^-20 max |ref64| over the rows (pre, g)"""
    r32 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 1, 1.0, dtype=np.float32)[2]
    r64 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 1, 1.0, dtype=np.float64)[2]
    for k, (a, b32, b64) in enumerate(zip(H.split_params(got, dims), r32, r64)):
        tol = 4.0 * np.abs(b32.astype(np.float64) - b64).max() + 2.0 ** -20 * np.abs(b64).max()
        err = np.abs(a.astype(np.float64) - b64).max()
        assert err <= tol and np.any(b64 != 0), '%s: g_params[%d] error %.3g, tolerance %.3g' % (what, k, err, tol)


def test_facade_autograd_loss_and_example(capsys):
    import torch
    from env_build_amd import policy_grad
    from env_build_amd.grad import DifferentiableEnvironmentModel
    from env_build_amd.policy_rollout import policy_rollout_grad
    from tests._tape import load_example
    # 128 envs x 4 steps: 1 / (steps * B) and the mean-then-divide of the parent's loss are the same power of two, so both paths
    # push the same cotangents; 200 x 5 for the arrays
    task, N = 'left', 8
    obs_all, ref_all, net, scale = H.scene(task, N, 64, 2)
    D, layers, dims = net[0], net[6], net[:4]
    dev = H.model(task, N)
    model = DifferentiableEnvironmentModel(task, 0, mode='training', n_veh=N)

    def make(precision='fp32'):
        pol = policy_grad.TrainableMLPNet(D, 2, 64, 'elu', 4, name='policy', output_activation='linear', precision=precision)
        pol.set_weights([a for pair in layers for a in pair])
        pol.set_obs_scale(scale)
        return pol
    pol = make()
    m = dev.make_mlp(*net, scale)
    names = {'out5': 'out5_steps', 'actions': 'actions_steps', 'obs': 'obs_steps', 'last': 'obs', 'cost': 'cost', 'g_actions': 'g_actions_steps',
             'g_obs0': 'g_obs0'}
    want = ('out5', 'actions', 'obs', 'cost', 'g_actions', 'g_obs0', 'g_params')
    B, steps = 200, 5
    obs0, ref_idx = obs_all[:B], ref_all[:B]
    w5 = tuple(v / (steps * B) for v in W5)
    ref = H.loop(dev, m, obs0, steps, w5, ref_idx)
    fused = policy_rollout_grad(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=want)
    composed = policy_rollout_grad(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=want, fused=False)
    assert fused['fused'] is True and composed['fused'] is False
    pre, g = ref['pre'].reshape(steps * B, D), ref['g_actions'].reshape(steps * B, 2)
    for out in (fused, composed):
        H.assert_equal({k: out[v].numpy() for k, v in names.items()}, ref, 'facade, fused %s' % out['fused'])
        rule2(out['g_params'].numpy(), layers, pre, g, 'elu', scale, dims, 'facade, fused %s' % out['fused'])
    short = policy_rollout_grad(model, pol, obs0, steps, w5, ref_indexes=ref_idx)
    assert sorted(short) == ['cost', 'fused', 'g_params', 'obs'] and H.same(short['g_params'].numpy(), fused['g_params'].numpy())
    with pytest.raises(ValueError):
        policy_rollout_grad(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=('rewards',))
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        policy_rollout_grad(model, make('fp16'), obs0, steps, w5, ref_indexes=ref_idx, fused=True)

    # rollout_loss(...).backward() against the parent's autograd path on the same two objects
    adp = load_example('adp_policy_gradient')
    B, steps = 128, 4
    obs0, ref_idx = obs_all[:B], ref_all[:B]
    w5 = tuple(v / (steps * B) for v in W5)
    ref = H.loop(dev, m, obs0, steps, w5, ref_idx, g_params=True)
    pre, g = ref['pre'].reshape(steps * B, D), ref['g_actions'].reshape(steps * B, 2)
    ob, ri = torch.from_numpy(obs0).to(model.device), torch.from_numpy(ref_idx.astype(np.int32)).to(model.device)
    flat_grad = lambda: torch.cat([p.grad.reshape(-1) for p in pol.parameters()]).cpu().numpy()

    def clear():
        for p in pol.parameters():
            p.grad = None
    loss = policy_grad.rollout_loss(model, pol, ob, ri, steps, w5)
    loss.backward()
    got = flat_grad()
    assert H.same(got, ref['g_params'])                         # 128 envs: the one backward over the concatenated rows, bit for bit
    clear()
    loss_ref = adp.rollout_loss(model, lambda o: pol.mode(o, 1.0), ob, ri, steps, lam=10.0)
    loss_ref.backward()
    rule2(got, layers, pre, g, 'elu', scale, dims, 'rollout_loss')
    rule2(flat_grad(), layers, pre, g, 'elu', scale, dims, "the parent's autograd path")
    # the loss: both are float32 sums of the same 2 * steps * B products in another order; either is within (terms - 1) 2^-24 sum |terms|
    # of the exact sum
    terms = np.abs(ref['out5'][:, :2].astype(np.float64) * np.asarray(w5[:2], np.float64).reshape(1, 2, 1))
    assert abs(float(loss) - float(loss_ref)) <= 2 * terms.size * 2.0 ** -24 * terms.sum() and float(loss) != 0
    # an upstream factor scales the gradient; an Adam step is followed on the next call with no sync call
    clear()
    (4.0 * policy_grad.rollout_loss(model, pol, ob, ri, steps, w5)).backward()
    assert H.same(flat_grad(), 4.0 * got)
    torch.optim.Adam(pol.parameters(), lr=1e-3).step()
    after = policy_grad.rollout_loss(model, pol, ob, ri, steps, w5)
    new = pol.get_weights()
    m2 = dev.make_mlp(D, 2, 64, 4, 'elu', 'linear', list(zip(new[0::2], new[1::2])), scale)
    cost2 = torch.from_numpy(H.loop(dev, m2, obs0, steps, w5, ref_idx)['cost']).to(model.device)
    assert float(after) == float(cost2.sum()) and float(after) != float(loss)
    dev.api.mlp_destroy(m)
    dev.api.mlp_destroy(m2)
    torch.cuda.synchronize()
    # the example: adp_train_mlpnet.py's loop on the fused loss, both paths' first iteration printed
    capsys.readouterr()
    load_example('adp_train_fused').main(['256', '5', '3'])
    text = capsys.readouterr().out
    assert 'fused' in text and 'composed' in text and text.count('iter ') >= 3
