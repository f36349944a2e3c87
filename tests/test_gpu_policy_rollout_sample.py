"""GPU (-m gpu): the stochastic closed-loop rollout with its reparameterised gradient (env_build_amd/csrc/eb_policy_rollout_sample.hip,
include/envbuild_policy_rollout_sample.h) through the C-ABI and the façade.  The yardstick everywhere is
tests/_policy_rollout_sample.py's loop of existing single calls through the same two handles: (1) forward bit for bit, (2) eps = 0 is
eb_policy_rollout_grad's forward, (3) the reverse bit for bit, (4) g_params bit for bit at multiples of 64 envs and within rule (2) of
DESIGN §17 elsewhere, (5) repeatability and row independence, (6) refusals, (7) side streams and capture — the obligations of
tests/test_stream_census.py's table, which does not count an entry whose stream is a struct field — (8) the façade, the autograd loss
and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from env_build_amd import _capi, policy_rollout as PR  # noqa: E402
from env_build_amd.policy_grad import mlp_backward_reference  # noqa: E402
from env_build_amd.policy_sample import policy_noise_reference  # noqa: E402
from tests import _capture, _policy, _policy_rollout_grad as G, _policy_rollout_sample as H  # noqa: E402
from tests._policy import F16, F32  # noqa: E402
from tests._policy_cases import make_layers  # noqa: E402

pytestmark = pytest.mark.gpu
W5 = H.W5
#        task, N, units, hidden layers, hidden activation: one per instantiation width and task
CASES = [('left', 8, 256, 2, 'elu'), ('right', 5, 64, 1, 'relu'), ('straight', 32, 128, 3, 'tanh')]
IDS = lambda c: '%s_N%d_%dx%d_%s' % (c[0], c[1], c[3], c[2], c[4])       # noqa: E731
SEED, given_noise = H.SEED, H.given_noise


# ---- 1: forward == the loop (the body: tests/_policy_rollout_sample.forward_equals_the_loop) ----
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_equals_the_loop(case):
    H.forward_equals_the_loop(case, sizes=(1, 63, 64, 65, 200), horizons=(1, 5), long=25, others=True)


# ---- 2: eps = 0 is the deterministic rollout ----
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_zero_noise_gives_the_deterministic_rollouts_forward(case):
    """x = fma(std, 0, mean) is the mean as a number (a zero's sign may differ), so every forward output equals
    eb_policy_rollout_grad's as numbers"""
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = H.scene(task, N, units, n_hidden, hact=hact)
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    for ar in (1.0, 0.5):
        det = G.entry(dev, m, obs0, 5, W5, ref_idx, ar=ar, want=('last', 'out5', 'actions', 'obs', 'cost'))
        got = H.entry(dev, m, obs0, 5, W5, ref_idx=ref_idx, ar=ar, eps=np.zeros((5, 200, 2), np.float32), want=H.FORWARD)
        for k, v in det.items():
            assert np.array_equal(got[k], v), (case, ar, k)
    dev.api.mlp_destroy(m)


# ---- 3: the reverse == the loop (the body: tests/_policy_rollout_sample.reverse_equals_the_loop) ----
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reverse_equals_the_loop(case):
    H.reverse_equals_the_loop(case, sizes=(1, 65, 200), horizons=(1, 5))


# ---- 4: g_params ----
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_g_params_equal_one_backward_over_the_concatenated_rows(case):
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = H.scene(task, N, units, n_hidden, hact=hact)
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    for B in (64, 128):
        for steps in (1, 5):
            w5 = tuple(v / (steps * B) for v in W5)
            kw = dict(w_logp=0.3 / (steps * B), ref_idx=ref_idx[:B], seed=SEED)
            ref = H.loop(dev, m, obs0[:B], steps, w5, g_params=True, **kw)
            got = H.entry(dev, m, obs0[:B], steps, w5, **kw)
            H.assert_equal(got, ref, '%s B=%d steps=%d' % (case, B, steps), H.PER_ROW + ('g_params',))
            assert np.any(ref['g_params'] != 0) and np.all(np.isfinite(ref['g_params']))
    dev.api.mlp_destroy(m)


def rule2(got, layers, pre, g, hact, scale, dims, what):
    """rule (2) of DESIGN §17 per parameter tensor: |got - ref64| <= 4 E + 2^-20 max |ref64| over the rows (pre, g), head 0
    -> the worst error / tolerance"""
    r32 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 0, 1.0, dtype=np.float32)[2]
    r64 = mlp_backward_reference(layers, pre, g, hact, 'linear', scale, 0, 1.0, dtype=np.float64)[2]
    worst = 0.0
    for k, (a, b32, b64) in enumerate(zip(H.split_params(got, dims), r32, r64)):
        tol = 4.0 * np.abs(b32.astype(np.float64) - b64).max() + 2.0 ** -20 * np.abs(b64).max()
        err = np.abs(a.astype(np.float64) - b64).max()
        print('%s: g_params[%d] error %.3g, tolerance %.3g' % (what, k, err, tol))
        assert err <= tol and np.any(b64 != 0), '%s: g_params[%d] error %.3g, tolerance %.3g' % (what, k, err, tol)
        worst = max(worst, float(err / tol))
    return worst


@pytest.mark.parametrize('case', [CASES[0], CASES[2]], ids=IDS)
def test_g_params_within_the_bound_at_ragged_batch_sizes(case):
    """per tensor |g_params - ref64| <= 4 E + 2^-20 max |ref64|: ref64 = mlp_backward_reference(float64, head 0) over the concatenated
    rows with the kernel's own obs_t and g_y_t (the loop's, which test 3 holds equal bit for bit and this test again), E the float32
    restatement's distance from it.  Measured worst error / tolerance: DESIGN §21."""
    task, N, units, n_hidden, hact = case
    obs0, ref_idx, net, scale = H.scene(task, N, units, n_hidden, hact=hact)
    dims, layers = net[:4], net[6]
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    steps, worst = 5, 0.0
    for B in (1, 65, 200):
        w5 = tuple(v / (steps * B) for v in W5)
        kw = dict(w_logp=0.3 / (steps * B), ref_idx=ref_idx[:B], seed=SEED)
        ref = H.loop(dev, m, obs0[:B], steps, w5, **kw)
        got = H.entry(dev, m, obs0[:B], steps, w5, **kw)
        H.assert_equal(got, ref, '%s B=%d' % (case, B), H.PER_ROW)
        worst = max(worst, rule2(got['g_params'], layers, ref['pre'].reshape(steps * B, -1), ref['g_y'].reshape(steps * B, 4), hact, scale,
                                 dims, '%s B=%d' % (case, B)))
    print('%s: worst error / tolerance %.3f' % (case, worst))
    dev.api.mlp_destroy(m)


# ---- 5: rows, calls ----
def test_calls_repeat_and_rows_are_independent():
    task, N = 'left', 8
    obs0, ref_idx, net, scale = H.scene(task, N, 256, 2)
    dev = H.model(task, N)
    m = dev.make_mlp(*net, scale)
    B = len(obs0)
    kw = dict(w_logp=0.3, seed=SEED, counter=3)
    first = H.entry(dev, m, obs0, 5, W5, ref_idx=ref_idx, **kw)
    H.assert_equal(H.entry(dev, m, obs0, 5, W5, ref_idx=ref_idx, **kw), first, 'second call')
    perm = np.random.default_rng(5).permutation(B)
    H.assert_equal(H.rows_of(H.entry(dev, m, obs0[perm], 5, W5, ref_idx=ref_idx[perm], row_ids=perm, **kw), slice(None)),
                   H.rows_of(first, perm), 'permuted batch with its row ids')
    sl = np.arange(100, 171)
    H.assert_equal(H.rows_of(H.entry(dev, m, obs0[sl], 5, W5, ref_idx=ref_idx[sl], row_ids=sl, **kw), slice(None)), H.rows_of(first, sl),
                   'slice with its row ids')
    assert not H.same(H.entry(dev, m, obs0[sl], 5, W5, ref_idx=ref_idx[sl], want=('eps',), **kw)['eps'], first['eps'][:, sl])
    # non-finite values in two rows' egos: the loop's bits in those rows, every other row untouched
    bad = obs0.copy()
    bad[7, 3], bad[70, 4] = np.nan, np.inf
    got = H.entry(dev, m, bad, 5, W5, ref_idx=ref_idx, **kw)
    H.assert_equal(got, H.loop(dev, m, bad, 5, W5, ref_idx=ref_idx, **kw), 'non-finite rows', H.PER_ROW)
    keep = np.setdiff1d(np.arange(B), [7, 70])
    H.assert_equal(H.rows_of(got, keep), H.rows_of(first, keep), 'rows next to non-finite ones')
    assert not np.all(np.isfinite(got['last'][[7, 70]])) and not np.all(np.isfinite(got['g_params']))
    # a forward-only call needs no workspace (the header says so) and leaves one it is given alone
    assert H.workspace_bytes(dev, m, B, 5, 0) == 0 and H.workspace_bytes(dev, m, B, 5, 1) > 0
    fwd = H.entry(dev, m, obs0, 5, W5, ref_idx=ref_idx, want=H.FORWARD, ws_fill=H.SENTINEL, **kw)
    assert bool((fwd.pop('ws') == H.SENTINEL).all())
    H.assert_equal(fwd, first, 'forward only', H.FORWARD)
    # n_env = 0: zeros to g_params, nothing else
    torch = dev.torch
    g_par, other = torch.full((H.param_count(dev, m),), H.SENTINEL, device=dev.dev), torch.full((64,), H.SENTINEL, device=dev.dev)
    o = H.raw(other)
    H.call(dev, m, n_env=0, steps=5, action_range=1.0, w5=W5, obs_out=o, out5_steps=o, actions_steps=o, obs_steps=o, cost=o, logp_steps=o,
           eps_out_steps=o, g_actions_steps=o, g_obs0=o, g_params=H.raw(g_par), stream=dev.stream)
    assert bool((dev._ret(g_par) == 0).all()) and bool((dev._ret(other) == H.SENTINEL).all())
    H.call(dev, m, n_env=0, steps=5, action_range=1.0, stream=dev.stream)
    assert H.workspace_bytes(dev, m, 0, 5) == 0
    dev.api.mlp_destroy(m)


# ---- 6: what the kernel takes, and the refusals ----
def refused(dev, m, obs, match, ref_idx=None, exc=ValueError, **kw):
    """eb_policy_rollout_sample raises with `match` in the message and writes nothing"""
    torch = dev.torch
    ob, ri = dev._in(obs), dev._in(ref_idx, np.int32)
    n, D = ob.shape
    steps = kw.pop('steps', 5)
    shp = H.shapes(n, D, min(max(steps, 1), 5), 70000)
    outs = [torch.empty(shp[k], device=dev.dev) for k in H.OUTPUTS]
    ws = torch.empty((1 << 22,), device=dev.dev)
    fields = dict(n_env=n, steps=steps, path_id=0, action_range=1.0, w_logp=0.1, w5=W5, obs_in=H.raw(ob), ref_idx=H.raw(ri),
                  workspace_bytes=ws.numel() * 4, stream=dev.stream)
    fields.update(kw)

    def run(w, *o):
        f = dict(fields, workspace=w.value, **{H.FIELD[k]: p.value for k, p in zip(H.OUTPUTS, o)})
        if kw.get('alias'):
            f['obs_out'] = f['obs_in']
        f.pop('alias', None)
        H.call(dev, m, **f)
    _policy.refused(dev, run, [ws] + outs, match, exc)
    assert H.same(dev._ret(ob), np.ascontiguousarray(obs, np.float32))


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
    fut = G.TapeModel('left', n_veh=8, n_future=1)
    cases.append((fut, net(fut.D, 256, 4), 'n_future 1 is not supported'))
    for model, m, reason in cases:
        ok, why = H.supported(model, m)
        assert ok == 0 and reason in why and 'eb_policy_rollout_sample' in why, (reason, why)
        refused(model, m, rng.standard_normal((70, model.D)).astype(np.float32), reason, ref_idx=ri)
        with pytest.raises(ValueError, match=reason):
            H.workspace_bytes(model, m, 70, 5)
        dev.api.mlp_destroy(m)
    sup = H.fn(dev, 'eb_policy_rollout_sample_supported')
    for args, match in (((None, good, C.byref(C.c_int32())), 'eb_policy_rollout_sample_supported: null handle'),
                        ((dev.h, None, C.byref(C.c_int32())), 'eb_policy_rollout_sample_supported: null policy'),
                        ((dev.h, good, None), 'null output pointer')):
        with pytest.raises(ValueError, match=match):
            dev.api.check(sup(*args))
    refused(dev, None, obs, 'eb_policy_rollout_sample: null policy', ref_idx=ri)
    refused(dev, good, obs, 'struct_size is 8', ref_idx=ri, struct_size=8)
    cap = PR.POLICY_ROLLOUT_SAMPLE_MAX_STEPS
    refused(dev, good, obs, 'steps 0 is outside 1 .. %d' % cap, ref_idx=ri, steps=0)
    refused(dev, good, obs, 'steps %d is outside 1 .. %d' % (cap + 1, cap), ref_idx=ri, steps=cap + 1)
    refused(dev, good, obs, 'n_env < 0', ref_idx=ri, n_env=-1)
    refused(dev, good, obs, 'rows, one row reduction takes', ref_idx=ri, n_env=2 ** 31 - 64, steps=cap)
    refused(dev, good, obs, 'training mode needs ref_idx')
    refused(dev, good, obs, 'action_range or w_logp is NaN', ref_idx=ri, action_range=float('nan'))
    refused(dev, good, obs, 'action_range or w_logp is NaN', ref_idx=ri, w_logp=float('nan'))
    need = H.workspace_bytes(dev, good, 70, 5)
    assert need % 4 == 0 and need < (1 << 24)
    refused(dev, good, obs, 'the workspace holds %d bytes' % (need - 4), ref_idx=ri, workspace_bytes=need - 4)
    refused(dev, good, obs, 'obs_out must not alias obs_in', ref_idx=ri, alias=True)
    refused(dev, good, obs, 'null obs_in', ref_idx=ri, obs_in=None)
    sel = H.model('left', 8, 'selecting')
    refused(sel, good, obs, 'bad path_id', path_id=3)
    refused(sel, good, obs, 'bad path_id', path_id=-1)
    with pytest.raises(ValueError, match='null workspace with a gradient asked for'):
        g = dev._out((70, 9))
        H.call(dev, good, n_env=70, steps=5, action_range=1.0, w5=W5, obs_in=H.raw(dev._in(obs)), ref_idx=H.raw(dev._in(ri, np.int32)),
               g_obs0=H.raw(g), stream=dev.stream)
    with pytest.raises(ValueError, match='eb_policy_rollout_sample: null handle'):
        a = PR.sample_args(n_env=70, steps=5)
        dev.api.check(H.fn(dev, 'eb_policy_rollout_sample')(None, good, C.byref(a)))
    with pytest.raises(ValueError, match='eb_policy_rollout_sample: null args'):
        dev.api.check(H.fn(dev, 'eb_policy_rollout_sample')(dev.h, good, None))
    # EB_ESTATE: a policy whose layers were never set
    cfg = _capi.EbMlpConfig(_capi.EB_ABI_VERSION, D, 2, 256, 4, _capi.ACT_ID['elu'], _capi.ACT_ID['linear'], 0)
    bare = C.c_void_p()
    dev.api.check(dev.api.lib.eb_mlp_create(C.byref(cfg), C.byref(bare)))
    ok, why = H.supported(dev, bare)
    assert ok == 0 and 'a layer was never set' in why
    refused(dev, bare, obs, 'a layer was never set', ref_idx=ri, exc=_capi.EbError)
    dev.api.mlp_destroy(bare)
    assert H.fn(dev, 'eb_policy_rollout_sample_abi_version')() == PR.EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION == 1
    dev.api.mlp_destroy(good)


# ---- 7: streams and capture ----
@pytest.mark.parametrize('B', [65, 200])
@pytest.mark.parametrize('steps', [1, 5])
def test_side_stream_and_capture(B, steps):
    """what tests/test_gpu_capture.py asks of a stream-taking entry: the null stream's bits on a side stream; under capture nothing runs,
    the graph is one chain of exactly 1 kernel node forward-only and 3 with g_params, no memset or memcpy node; two replays with other
    input contents equal two eager calls.  w5, w_logp, seed and counter are read at call time (the header says so): the replays keep the
    captured ones."""
    task, N = 'left', 8
    obs_all, ref_all, net, scale = H.scene(task, N, 64, 2)
    dev = H.model(task, N)
    torch = dev.torch
    m = dev.make_mlp(*net, scale)
    obs0, ref_idx = obs_all[:B], ref_all[:B]
    w5 = tuple(v / (steps * B) for v in W5)
    kw = dict(w_logp=0.3 / (steps * B), ref_idx=ref_idx, seed=SEED, counter=11)
    eager = H.entry(dev, m, obs0, steps, w5, **kw)
    side = _capture.side_stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = H.entry(dev, m, obs0, steps, w5, stream=side.cuda_stream, **kw)
    side.synchronize()
    H.assert_equal(on_side, eager, 'side stream')
    other = obs_all[200 - B:200].copy()
    other[:, 3] += np.float32(0.25)
    eager2 = H.entry(dev, m, other, steps, w5, **kw)
    D, count = obs0.shape[1], H.param_count(dev, m)
    for want, kernels in ((H.FORWARD, 1), (H.OUTPUTS, 3)):
        ob, ri = dev._in(obs0), dev._in(ref_idx, np.int32)
        need = H.workspace_bytes(dev, m, B, steps, int(kernels == 3))
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev.dev)
        bufs = {k: torch.full(s, H.SENTINEL, device=dev.dev) for k, s in H.shapes(B, D, steps, count).items() if k in want}
        fields = dict(n_env=B, steps=steps, action_range=1.0, w_logp=kw['w_logp'], w5=w5, seed=SEED, counter=11, obs_in=H.raw(ob),
                      ref_idx=H.raw(ri), workspace=H.raw(ws) if need else None, workspace_bytes=need,
                      **{H.FIELD[k]: H.raw(v) for k, v in bufs.items()})
        torch.cuda.synchronize()
        g = _capture.capture(side, lambda raw_stream: H.call(dev, m, stream=raw_stream, **fields), 'eb_policy_rollout_sample')
        try:
            torch.cuda.synchronize()
            assert all(bool((v == H.SENTINEL).all()) for v in bufs.values()), 'the capture ran something'
            kinds = g.node_types()
            assert kinds == {'kernel': kernels} and g.is_chain(), (dict(kinds), kernels)
            for src, ref in ((obs0, eager), (other, eager2)):
                ob.copy_(torch.from_numpy(src))
                torch.cuda.synchronize()
                g.replay()
                side.synchronize()
                H.assert_equal({k: dev._ret(v) for k, v in bufs.items()}, ref, 'replay, %d kernels' % kernels)
        finally:
            g.close()
    dev.api.mlp_destroy(m)


# ---- 8: façade, autograd, example ----
def test_facade_autograd_loss_and_example(capsys):
    import torch
    from env_build_amd import policy_grad
    from env_build_amd.grad import DifferentiableEnvironmentModel
    from env_build_amd.policy_rollout import policy_rollout_sample
    from tests._tape import load_example
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
    names = {'out5': 'out5_steps', 'actions': 'actions_steps', 'obs': 'obs_steps', 'last': 'obs', 'cost': 'cost', 'logp': 'logp_steps',
             'eps': 'eps_steps', 'g_actions': 'g_actions_steps', 'g_obs0': 'g_obs0'}
    B, steps = 200, 5
    obs0, ref_idx = obs_all[:B], ref_all[:B]
    w5 = tuple(v / (steps * B) for v in W5)
    w_logp = 0.3 / (steps * B)
    kw = dict(w_logp=w_logp, seed=SEED, counter=2)
    ref = H.loop(dev, m, obs0, steps, w5, ref_idx=ref_idx, **kw)
    pre, g = ref['pre'].reshape(steps * B, D), ref['g_y'].reshape(steps * B, 4)
    fused = policy_rollout_sample(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=PR.SAMPLE_WANT, **kw)
    composed = policy_rollout_sample(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=PR.SAMPLE_WANT, fused=False, **kw)
    assert fused['fused'] is True and composed['fused'] is False
    for out in (fused, composed):
        H.assert_equal({k: out[v].numpy() for k, v in names.items()}, ref, 'facade, fused %s' % out['fused'])
        rule2(out['g_params'].numpy(), layers, pre, g, 'elu', scale, dims, 'facade, fused %s' % out['fused'])
    short = policy_rollout_sample(model, pol, obs0, steps, **kw)
    assert sorted(short) == ['actions_steps', 'fused', 'logp_steps', 'obs'] and H.same(short['logp_steps'].numpy(), ref['logp'])
    with pytest.raises(ValueError):
        policy_rollout_sample(model, pol, obs0, steps, w5, ref_indexes=ref_idx, want=('rewards',))
    half = make('fp16')
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        policy_rollout_sample(model, half, obs0, steps, w5, ref_indexes=ref_idx, fused=True)
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        policy_rollout_sample(model, half, obs0, steps, w5, ref_indexes=ref_idx, want=('g_params',))
    low = policy_rollout_sample(model, half, obs0, steps, w5, ref_indexes=ref_idx, want=('actions', 'logp', 'eps'), **kw)
    assert low['fused'] is False and H.same(low['eps_steps'].numpy(), ref['eps']) and np.all(np.isfinite(low['logp_steps'].numpy()))

    # rollout_loss_sampled(...).backward() at 128 envs x 4 steps: the one backward over the concatenated rows, bit for bit
    B, steps = 128, 4
    obs0, ref_idx = obs_all[:B], ref_all[:B]
    w5 = tuple(v / (steps * B) for v in W5)
    w_logp = 0.25 / (steps * B)
    ref = H.loop(dev, m, obs0, steps, w5, w_logp=w_logp, ref_idx=ref_idx, seed=SEED, counter=9, g_params=True)
    ob, ri = torch.from_numpy(obs0).to(model.device), torch.from_numpy(ref_idx.astype(np.int32)).to(model.device)
    flat_grad = lambda: torch.cat([p.grad.reshape(-1) for p in pol.parameters()]).cpu().numpy()

    def clear():
        for p in pol.parameters():
            p.grad = None
    loss = policy_grad.rollout_loss_sampled(model, pol, ob, ri, steps, w5, w_logp, SEED, 9)
    loss.backward()
    got = flat_grad()
    assert H.same(got, ref['g_params'])
    # the loss: a float32 sum of the 2 * steps * B weighted out5 terms and the steps * B weighted logp terms in some order: within
    # (terms - 1) 2^-24 sum |terms| of the exact sum, twice that between two such sums (§18's test states the same bound)
    terms = np.concatenate([np.abs(ref['out5'][:, :2].astype(np.float64) * np.asarray(w5[:2], np.float64).reshape(1, 2, 1)).ravel(),
                            np.abs(ref['logp'].astype(np.float64) * w_logp).ravel()])
    exact = float((ref['out5'][:, :2].astype(np.float64) * np.asarray(w5[:2], np.float64).reshape(1, 2, 1)).sum()
                  + (ref['logp'].astype(np.float64) * np.float64(np.float32(w_logp))).sum())
    assert abs(float(loss.detach()) - exact) <= 2 * terms.size * 2.0 ** -24 * terms.sum() and float(loss.detach()) != 0
    # an upstream factor scales the gradient; an Adam step is followed on the next call with no sync call
    clear()
    (4.0 * policy_grad.rollout_loss_sampled(model, pol, ob, ri, steps, w5, w_logp, SEED, 9)).backward()
    assert H.same(flat_grad(), 4.0 * got)
    torch.optim.Adam(pol.parameters(), lr=1e-3).step()
    after, logp = policy_grad.rollout_loss_sampled(model, pol, ob, ri, steps, w5, w_logp, SEED, 9, return_logp=True)
    new = pol.get_weights()
    m2 = dev.make_mlp(D, 2, 64, 4, 'elu', 'linear', list(zip(new[0::2], new[1::2])), scale)
    ref2 = H.loop(dev, m2, obs0, steps, w5, w_logp=w_logp, ref_idx=ref_idx, seed=SEED, counter=9, grad=False)
    assert H.same(logp.cpu().numpy(), ref2['logp']) and not H.same(ref2['logp'], ref['logp']) and float(after.detach()) != float(loss.detach())
    dev.api.mlp_destroy(m)
    dev.api.mlp_destroy(m2)
    torch.cuda.synchronize()
    # the example: adp_train_fused.py's loop on the sampled loss, both paths' first iteration printed
    capsys.readouterr()
    load_example('adp_train_maxent').main(['256', '5', '3'])
    text = capsys.readouterr().out
    assert 'fused' in text and 'composed' in text and 'mean logp' in text and text.count('iter ') >= 3
