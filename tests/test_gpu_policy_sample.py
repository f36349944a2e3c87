"""GPU (-m gpu): the stochastic policy head (include/envbuild_policy_sample.h) — the two elementwise entries against the float32
restatement bit for bit, the fused launch against eb_mlp_forward followed by the epilogue, eps = 0 against eb_policy_run_batch, row
independence, `sample` on a TrainableMLPNet against the float64 torch twin, the fp16 route, Policy4Toyota's stochastic branch and the
example loop."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from env_build_amd import policy_sample as ps
from env_build_amd.policy_grad import mlp_backward_reference
from tests._helpers import ROOT
from tests._policy import SENTINEL, same
from tests._policy_cases import HOST_CONFIGS, make_layers

pytestmark = pytest.mark.gpu

RANGES = (1.0, 0.5, None)
N_MAX = 300
SEED, COUNTER = 0x1234567, 5


def gpu(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host(d):
    import torch
    torch.cuda.synchronize()
    return {k: v.numpy() for k, v in d.items()}


# ---- 1: the elementwise entries against the restatement -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logits_case(out_dim):
    """N_MAX rows of logits with their eps and cotangents: the pre-tanh value on both sides of 0.625 and 44 (rows 0..15, eps = 0 there, so
    x is the mean), log-std from -20 to 5, row 20 all NaN, row 22 with +inf / -inf, the rest random"""
    rng = np.random.default_rng(out_dim)
    act_dim = out_dim // 2
    mean = (1.5 * rng.standard_normal((N_MAX, act_dim))).astype(np.float32)
    ls = rng.uniform(-4.0, 1.0, (N_MAX, act_dim)).astype(np.float32)
    eps = rng.standard_normal((N_MAX, act_dim)).astype(np.float32)
    edge = np.array([0.6, 0.625, 0.65, -0.6, -0.625, -0.65, 43.9, 44.0, 44.1, -43.9, -44.0, -44.1, 0.0, -0.0, 90.0, -90.0], np.float32)
    mean[:16] = edge[:, None]
    eps[:16] = 0.0
    ls[24:24 + 26] = np.linspace(-20.0, 5.0, 26, dtype=np.float32)[:, None]
    ls[50:56] = np.array([-100.0, -87.5, 88.5, 100.0, 5.0, -20.0], np.float32)[:, None]
    eps[56:60] = np.array([5.77, -5.77, 1e-30, -0.0], np.float32)[:, None]
    mean[20], ls[20] = np.nan, np.nan
    mean[22, 0], ls[22, -1] = np.inf, -np.inf
    if act_dim > 1:
        mean[22, 1] = -np.inf
    g_a = rng.standard_normal((N_MAX, act_dim)).astype(np.float32)
    g_lp = rng.standard_normal(N_MAX).astype(np.float32)
    return np.concatenate([mean, ls], axis=1), eps, g_a, g_lp


@functools.lru_cache(maxsize=None)
def reference(out_dim, action_range, drawn):
    """the float32 restatement for all N_MAX rows, computed once: rows are independent, so a smaller n is its first rows"""
    logits, eps, g_a, g_lp = logits_case(out_dim)
    if drawn:
        eps = ps.policy_noise_reference(np.arange(N_MAX), out_dim // 2, SEED, COUNTER)
    actions, logp, g_logits = ps.policy_sample_reference(logits, eps, action_range, g_a, g_lp)
    only_a = ps.policy_sample_reference(logits, eps, action_range, g_a, None)[2]
    only_lp = ps.policy_sample_reference(logits, eps, action_range, None, g_lp)[2]
    return dict(actions=actions, logp=logp, eps=eps, g_logits=g_logits, g_only_a=only_a, g_only_lp=only_lp)


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('out_dim', [2, 4, 6, 32])
def test_from_logits_and_vjp_are_the_restatement_bit_for_bit(out_dim, action_range):
    logits, eps, g_a, g_lp = logits_case(out_dim)
    for n in (1, 63, 64, 65, N_MAX):
        y = gpu(logits[:n])
        for drawn in (False, True):
            want = reference(out_dim, action_range, drawn)
            got = host(ps.sample_from_logits(y, action_range, None if drawn else eps[:n], SEED, COUNTER, want=('logp', 'eps')))
            for k in ('actions', 'logp', 'eps'):
                assert same(got[k], want[k][:n]), '%s differs, n %d, drawn %s' % (k, n, drawn)
            e = gpu(want['eps'][:n])
            for key, ga, gl in (('g_logits', g_a[:n], g_lp[:n]), ('g_only_a', g_a[:n], None), ('g_only_lp', None, g_lp[:n])):
                g = ps.sample_vjp(y, e, action_range, ga, gl).numpy()
                assert same(g, want[key][:n]), '%s differs, n %d, drawn %s' % (key, n, drawn)
    # the poisoned rows poison themselves only
    want = reference(out_dim, action_range, False)
    assert np.isnan(want['logp'][20]) and np.isnan(want['actions'][20]).all()
    assert not np.isfinite(want['logp'][22])
    clean = np.ones(N_MAX, bool)
    clean[[20, 22]] = False
    clean[50:56] = False              # log-std beyond the exponential's clamps: std * eps may overflow, compared bit for bit above
    assert np.isfinite(want['logp'][clean]).all() and np.isfinite(want['actions'][clean]).all()


def test_from_logits_optional_outputs_and_row_ids():
    import torch
    logits, eps, _, _ = logits_case(4)
    api = ps._capi.hip_api()
    fn = ps.bind(api)['eb_policy_sample_from_logits']
    y = gpu(logits)
    ids = np.random.default_rng(9).permutation(N_MAX).astype(np.int32)
    ids[0] = -1                                                             # 2^32 - 1 as an unsigned number
    actions = torch.full((N_MAX, 2), SENTINEL, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    api.check(fn(N_MAX, 4, y.data_ptr(), None, gpu(ids, np.int32).data_ptr(), SEED, COUNTER, 1.0, actions.data_ptr(), None, None, stream))
    want_eps = ps.policy_noise_reference(ids, 2, SEED, COUNTER)
    want = ps.policy_sample_reference(logits, want_eps, 1.0)
    torch.cuda.synchronize()
    assert same(actions.cpu().numpy(), want[0])
    got = host(ps.sample_from_logits(y, 1.0, None, SEED, COUNTER, row_ids=ids, want=('logp', 'eps')))
    assert same(got['eps'], want_eps) and same(got['logp'], want[1])
    # n = 0 writes nothing
    api.check(fn(0, 4, y.data_ptr(), None, None, SEED, COUNTER, 1.0, actions.data_ptr(), None, None, stream))
    with pytest.raises(ValueError, match='eb_policy_sample_from_logits'):
        api.check(fn(4, 3, y.data_ptr(), None, None, SEED, COUNTER, 1.0, actions.data_ptr(), None, None, stream))


# ---- 2: the fused launch against eb_mlp_forward followed by the epilogue ---------------------------------------------------------------
FUSED_CONFIGS = [c for c in HOST_CONFIGS if c[3] % 2 == 0] + [
    # one width each of 64 / 128 / 256 / 512: the four instantiations; out_dim 18: a partly filled second column tile
    (20, 1, 64, 8, 'elu', 'linear'), (20, 2, 128, 16, 'tanh', 'linear'), (20, 1, 256, 18, 'relu', 'tanh'), (20, 1, 512, 2, 'elu', 'linear')]


def make_net(cfg, scale, cls=None, **kw):
    from env_build_amd.policy import MLPNet
    obs_dim, n_hidden, n_units, out_dim, hact, oact = cfg
    rng = np.random.default_rng(sum(cfg[:4]))
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim, bias_scale=0.3)
    net = (cls or MLPNet)(obs_dim, n_hidden, n_units, hact, out_dim, output_activation=oact, **kw)
    net.set_weights([a for pair in layers for a in pair])
    sc = rng.uniform(0.25, 1.0, obs_dim).astype(np.float32) if scale else None
    if scale:
        net.set_obs_scale(sc)
    return net, layers, sc


@pytest.mark.parametrize('cfg', FUSED_CONFIGS, ids=['%dx%dx%dx%d' % c[:4] for c in FUSED_CONFIGS])
def test_fused_equals_forward_then_from_logits(cfg):
    import torch
    obs_dim, out_dim = cfg[0], cfg[3]
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((129, obs_dim)).astype(np.float32)
    eps = rng.standard_normal((129, out_dim // 2)).astype(np.float32)
    for scale in (False, True):
        net, _, _ = make_net(cfg, scale)
        ok = C.c_int32(0)
        ps._call(net.api, 'eb_policy_sample_supported', net._handle, C.byref(ok))
        assert ok.value == 1
        for n in (1, 65, 129):
            logits = net.call(obs[:n])
            for ar in RANGES:
                for given in (None, eps[:n]):
                    want = host(ps.sample_from_logits(logits, ar, given, SEED, COUNTER, want=('logp', 'eps')))
                    got = host(ps.sample_actions(net, obs[:n], ar, given, SEED, COUNTER, want=('logp', 'logits', 'eps')))
                    assert same(got['logits'], logits.numpy()), 'logits_out, n %d' % n
                    for k in ('actions', 'logp', 'eps'):
                        assert same(got[k], want[k]), '%s, n %d, range %r, eps %s' % (k, n, ar, 'drawn' if given is None else 'given')
        # every optional output NULL: the actions alone, and nothing beyond them
        out = torch.full((129 + 1, out_dim // 2), SENTINEL, device='cuda')
        x = gpu(obs)
        ps._call(net.api, 'eb_policy_sample', net._handle, 129, x.data_ptr(), None, None, SEED, COUNTER, 1.0, out.data_ptr(), None, None,
                 None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert same(out[:129].cpu().numpy(), host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER))['actions'])
        assert bool((out[129] == SENTINEL).all())


# ---- 3: zero noise is the deterministic action ------------------------------------------------------------------------------------------
def test_zero_noise_gives_the_deterministic_action():
    cfg = (41, 2, 256, 4, 'elu', 'linear')
    net, layers, _ = make_net(cfg, True)
    rng = np.random.default_rng(2)
    obs = rng.standard_normal((200, 41)).astype(np.float32)
    zeros = np.zeros((200, 2), np.float32)
    for ar in RANGES:
        got = host(ps.sample_actions(net, obs, ar, zeros))['actions']
        assert np.array_equal(got, net.mode(obs, ar).numpy()), ar
    # mean = -0.0 is the one value whose zero changes sign: x = fmaf(std, 0, -0.0) is +0.0
    y = gpu(np.array([[-0.0, 0.5]], np.float32))
    a = ps.sample_from_logits(y, 1.0, np.zeros((1, 1), np.float32))['actions'].numpy()
    assert a[0, 0] == 0.0 and not np.signbit(a[0, 0])


# ---- 4: rows are independent, calls repeat, n = 0 writes nothing ------------------------------------------------------------------------
def test_rows_are_independent_and_calls_repeat():
    import torch
    cfg = (137, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True)
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((N_MAX, 137)).astype(np.float32)
    want = ('logp', 'logits', 'eps')
    full = host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER, want=want))
    again = host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER, want=want))
    for k in full:
        assert same(full[k], again[k]), k
    assert not same(full['eps'], host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER + 1, want=want))['eps'])
    assert not same(full['eps'], host(ps.sample_actions(net, obs, 1.0, None, SEED + 1, COUNTER, want=want))['eps'])
    for row in (0, 63, 64, 200, N_MAX - 1):
        one = host(ps.sample_actions(net, obs[row:row + 1], 1.0, None, SEED, COUNTER, row_ids=np.array([row]), want=want))
        for k in full:
            assert same(one[k], full[k][row:row + 1]), '%s, row %d' % (k, row)
    # n = 0: nothing is written
    out = torch.full((4, 2), SENTINEL, device='cuda')
    lp = torch.full((4,), SENTINEL, device='cuda')
    ps._call(net.api, 'eb_policy_sample', net._handle, 0, None, None, None, SEED, COUNTER, 1.0, out.data_ptr(), lp.data_ptr(), None, None,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((lp == SENTINEL).all())
    empty = ps.sample_actions(net, np.zeros((0, 137), np.float32), 1.0)
    assert empty['actions'].numpy().shape == (0, 2) and empty['logp'].numpy().shape == (0,)


# ---- 5: the autograd node against the float64 torch twin --------------------------------------------------------------------------------
def twin(layers, obs, eps, hact, oact, scale, action_range, g_a, g_lp):
    """float64: _policy_cases.torch_twin's layers under torch.distributions, same eps -> (actions, logp, g_obs, g_params)"""
    import torch
    from torch import distributions as D
    acts = {'linear': lambda x: x, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh}
    params = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for pair in layers for a in pair]
    x0 = torch.tensor(np.asarray(obs, np.float64), requires_grad=True)
    x = x0 if scale is None else x0 * torch.tensor(np.asarray(scale, np.float64))
    for L in range(len(layers)):
        x = acts[oact if L == len(layers) - 1 else hact](x @ params[2 * L] + params[2 * L + 1])
    act_dim = x.shape[1] // 2
    mean, ls = x[:, :act_dim], x[:, act_dim:]
    base = D.Independent(D.Normal(mean, ls.exp()), 1)
    pre = mean + ls.exp() * torch.tensor(np.asarray(eps, np.float64))
    if action_range is None:
        actions, logp = pre, base.log_prob(pre)
    else:
        tanh = D.transforms.TanhTransform(cache_size=1)
        affine = D.transforms.AffineTransform(0.0, float(action_range), cache_size=1)
        actions = affine(tanh(pre))
        logp = D.TransformedDistribution(base, [tanh, affine]).log_prob(actions)
    ((actions * torch.tensor(np.asarray(g_a, np.float64))).sum() + (logp * torch.tensor(np.asarray(g_lp, np.float64))).sum()).backward()
    return actions.detach().numpy(), logp.detach().numpy(), x0.grad.numpy(), [p.grad.numpy() for p in params]


def restatement32(layers, obs, eps, hact, oact, scale, action_range, g_a, g_lp):
    """the same in float32, from the two NumPy restatements"""
    logits = mlp_backward_reference(layers, obs, np.zeros((len(obs), layers[-1][0].shape[1]), np.float32), hact, oact, scale, 0)[0]
    actions, logp, g_logits = ps.policy_sample_reference(logits, eps, action_range, g_a, g_lp)
    _, g_obs, g_params = mlp_backward_reference(layers, obs, g_logits, hact, oact, scale, 0)
    return actions, logp, g_obs, g_params


def bound_failures(got, r32, r64, what):
    """tests/test_gpu_policy_grad.py's bar for eb_mlp_backward against its twin: per column of a [n, .] output and over a whole parameter
    tensor, |got - ref64| <= 4 E + 2^-20 max |ref64| with E = max |ref32 - ref64|"""
    tensors = [('actions', got[0], r32[0], r64[0], 0), ('logp', got[1], r32[1], r64[1], None), ('g_obs', got[2], r32[2], r64[2], 0)]
    tensors += [('g_params[%d]' % k, got[3][k], r32[3][k], r64[3][k], None) for k in range(len(r64[3]))]
    failures = []
    for name, a, b32, b64, axis in tensors:
        E = np.abs(b32.astype(np.float64) - b64).max(axis)
        tol = 4.0 * E + 2.0 ** -20 * np.abs(b64).max(axis)
        ratio = float((np.abs(a.astype(np.float64) - b64).max(axis) / np.maximum(tol, 1e-300)).max())
        print('%s %s: error / tolerance %.3f' % (what, name, ratio))
        if not ratio <= 1.0:
            failures.append((what, name, ratio))
    return failures


def test_sample_on_a_trainable_net_against_the_float64_twin():
    import torch
    from env_build_amd.policy_grad import TrainableMLPNet
    cfg = (41, 2, 100, 4, 'elu', 'linear')
    net, layers, scale = make_net(cfg, True, TrainableMLPNet)
    params = net.parameters()
    rng = np.random.default_rng(12)
    n = 200
    obs = rng.standard_normal((n, 41)).astype(np.float32)
    eps = rng.standard_normal((n, 2)).astype(np.float32)
    g_a, g_lp = rng.standard_normal((n, 2)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    zero_a, zero_lp = np.zeros_like(g_a), np.zeros_like(g_lp)
    failures = []
    for ar in RANGES:
        for what, ga, gl in (('both', g_a, g_lp), ('g_logp alone', None, g_lp), ('g_actions alone', g_a, None)):
            x = torch.from_numpy(obs).cuda().requires_grad_(True)
            for p in params:
                p.grad = None
            actions, logp = ps.sample(net, x, ar, eps=eps)
            assert actions.requires_grad and logp.requires_grad and actions.shape == (n, 2) and logp.shape == (n,)
            loss = 0.0
            if ga is not None:
                loss = loss + (actions * torch.from_numpy(ga).cuda()).sum()
            if gl is not None:
                loss = loss + (logp * torch.from_numpy(gl).cuda()).sum()
            loss.backward()
            got = (actions.detach().cpu().numpy(), logp.detach().cpu().numpy(), x.grad.cpu().numpy(), [p.grad.cpu().numpy() for p in params])
            args = (layers, obs, eps, 'elu', 'linear', scale, ar, zero_a if ga is None else ga, zero_lp if gl is None else gl)
            failures += bound_failures(got, restatement32(*args), twin(*args), 'range %r, %s:' % (ar, what))
    assert not failures, failures
    # drawn noise: the node keeps what the launch drew; same (seed, counter), same sample; the forward equals sample_actions
    a1, l1 = ps.sample(net, obs, 1.0, seed=SEED, counter=COUNTER)
    ref = host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER))
    assert same(a1.detach().cpu().numpy(), ref['actions']) and same(l1.detach().cpu().numpy(), ref['logp'])
    (l1.sum() + a1.sum()).backward()
    # weights modified between forward and backward: refused, as call / mode do
    opt = torch.optim.SGD(params, lr=1e-3)
    a2, _ = ps.sample(net, obs, 1.0, seed=SEED, counter=COUNTER)
    opt.step()
    with pytest.raises(RuntimeError, match='modified in place'):
        a2.sum().backward()
    torch.cuda.synchronize()


# ---- 6: an fp16 handle ------------------------------------------------------------------------------------------------------------------
def test_an_fp16_handle_is_refused_by_the_fused_entry_and_served_by_the_epilogue():
    import torch
    cfg = (41, 2, 256, 4, 'elu', 'linear')
    net, _, _ = make_net(cfg, True, precision='fp16')
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((130, 41)).astype(np.float32)
    ok = C.c_int32(7)
    ps._call(net.api, 'eb_policy_sample_supported', net._handle, C.byref(ok))
    assert ok.value == 0 and b'EB_MLP_PRECISION_F32' in net.api.lib.eb_last_error()
    out = torch.full((130, 2), SENTINEL, device='cuda')
    x = gpu(obs)
    with pytest.raises(ValueError, match='eb_policy_sample: the handle.s precision must be EB_MLP_PRECISION_F32'):
        ps._call(net.api, 'eb_policy_sample', net._handle, 130, x.data_ptr(), None, None, SEED, COUNTER, 1.0, out.data_ptr(), None, None, None,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    logits = net.call(obs)
    want = host(ps.sample_from_logits(logits, 1.0, None, SEED, COUNTER, want=('logp', 'eps')))
    got = host(ps.sample_actions(net, obs, 1.0, None, SEED, COUNTER, want=('logp', 'logits', 'eps')))
    assert same(got['logits'], logits.numpy())
    for k in want:
        assert same(got[k], want[k]), k
    # any callable that returns logits takes the same route
    got = host(ps.sample_actions(lambda o: net.call(o), obs, 1.0, None, SEED, COUNTER, want=('logp', 'eps')))
    for k in want:
        assert same(got[k], want[k]), k


# ---- 7: the reference's API ---------------------------------------------------------------------------------------------------------------
def test_policy4toyota_stochastic_branch_and_load_policy():
    from types import SimpleNamespace
    from env_build_amd.policy import LoadPolicy, Policy4Toyota
    rng = np.random.default_rng(5)
    B, D = 70, 41
    obs = rng.standard_normal((B, D)).astype(np.float32)
    conf = dict(obs_dim=D, act_dim=2, num_hidden_layers=2, num_hidden_units=256, hidden_activation='elu', policy_out_activation='linear',
                action_range=1.0, obs_preprocess_type='scale', obs_scale=list(rng.uniform(0.25, 1.0, D)))
    pol = Policy4Toyota(SimpleNamespace(deterministic_policy=False, **conf))
    a1, l1 = pol.compute_action(obs)
    a2, l2 = pol.compute_action(obs)
    assert a1.numpy().shape == (B, 2) and l1.numpy().shape == (B,)
    assert not same(a1.numpy(), a2.numpy()) and np.abs(a1.numpy()).max() <= 1.0 and np.isfinite(l1.numpy()).all()
    pol.seed(77)
    b1, m1 = pol.compute_action(obs)
    b2, m2 = pol.compute_action(obs)
    pol.seed(77)
    c1, n1 = pol.compute_action(obs)
    c2, n2 = pol.compute_action(obs)
    assert same(b1.numpy(), c1.numpy()) and same(m1.numpy(), n1.numpy()) and same(b2.numpy(), c2.numpy()) and same(m2.numpy(), n2.numpy())
    ref = host(ps.sample_actions(pol.policy, obs, 1.0, None, 77, 1))
    assert same(b2.numpy(), ref['actions']) and same(m2.numpy(), ref['logp'])
    # LoadPolicy.run_batch follows the configuration
    sto = LoadPolicy(args=dict(deterministic_policy=False, **conf))
    det = LoadPolicy(args=dict(deterministic_policy=True, **conf))
    sto.policy.seed(3)
    r1 = sto.run_batch(obs).numpy()
    want = host(ps.sample_actions(sto.policy.policy, obs, 1.0, None, 3, 0))['actions']
    assert r1.shape == (B, 2) and same(r1, want) and not same(r1, sto.run_batch(obs).numpy())
    # the deterministic branch is what it was
    actions, logp = det.policy.compute_action(obs)
    assert logp == 0. and same(actions.numpy(), det.policy.compute_mode(obs).numpy())
    assert same(det.run_batch(obs).numpy(), det.policy.policy.mode(obs, 1.0).numpy())
    assert same(det.run_batch(obs).numpy(), sto.policy.compute_mode(obs).numpy())          # same seed, same weights


# ---- 8: the example -------------------------------------------------------------------------------------------------------------------------
def test_sample_env_loop_example_runs():
    spec = importlib.util.spec_from_file_location('sample_env_loop', os.path.join(ROOT, 'examples', 'sample_env_loop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.run(n_env=64, steps=5, warmup=1, num_hidden_units=64)
    assert set(out) == {'episodes', 'mean_return', 'mean_logp', 'steps_per_s'}
    assert np.isfinite(out['mean_logp']) and np.isfinite(out['mean_return']) and out['steps_per_s'] > 0
