"""GPU (-m gpu): the opt-in fp16 policy kernel (env_build_amd/csrc/eb_policy_f16.hip, include/envbuild_mlp_f16.h) through the C-ABI and
the façade.  Its sums take the matrix instruction's own order, so it is held to (1) the bits of the float64 restatement where every
partial sum is exact, (2) a per-column bound from the restatement's own fp32 / float64 runs on random networks, (3) leaving the fp32
path's bits alone, (4) row independence and repeatability, (5, 6) the shield as the generic loop gives it and the reference's G14 flags,
(7) clean refusals, (8) the façade."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from env_build_amd import _capi  # noqa: E402
from env_build_amd.policy import _tanh_det, mlp_f16_reference  # noqa: E402
from env_build_amd.synthetic import assemble_obs, make_rollout_inputs  # noqa: E402
from tests._grad_cases import column_tolerance  # noqa: E402
from tests._helpers import DeviceModel, HostModel, golden, oracle_lib, record_host  # noqa: E402
from tests._policy import F16, F32, f16_mlp, loop, loop_view, same, sparse_signs  # noqa: E402
from tests._policy_cases import CONFIGS, G14, make_layers  # noqa: E402

pytestmark = pytest.mark.gpu

# ---- 1: exact ----
EXACT_SHAPES = [(1, 1, 1, 1), (15, 1, 31, 2), (16, 2, 32, 4), (17, 2, 33, 17), (41, 2, 256, 4), (137, 2, 256, 4), (265, 2, 512, 4),
                (33, 4, 100, 6), (8, 8, 32, 2), (300, 1, 256, 32)]


def exact_chain(layers, obs, scale, relu):
    """float64 chain (every value exact there) -> (outputs, premise holds): every hidden activation representable in binary16 and, for
    every pre-activation, sum |products| / granularity < 2^20 — then fp32 sums are exact in ANY order"""
    gran = 2.0 ** -3
    x = obs.astype(np.float64) * (1.0 if scale is None else scale.astype(np.float64))
    ok = bool(np.all(x.astype(np.float16).astype(np.float64) == x))
    for L, (w, b) in enumerate(layers):
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        mass = np.abs(x) @ np.abs(w64) + np.abs(b64)
        pre = x @ w64 + b64
        ok = ok and bool(np.all(mass / gran < 2.0 ** 20)) and bool(np.all(np.round(pre / gran) == pre / gran))
        if L == len(layers) - 1:
            return pre, ok
        x = np.maximum(pre, 0.0) if relu else pre
        ok = ok and bool(np.all(x.astype(np.float16).astype(np.float64) == x))


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_exact_inputs_give_the_restatement_bits(shape):
    obs_dim, n_hidden, n_units, out_dim = shape
    relu = EXACT_SHAPES.index(shape) % 2 == 0
    rng = np.random.default_rng(obs_dim * 31 + n_units)
    dev = DeviceModel('left')
    dims = [obs_dim] + [n_units] * n_hidden + [out_dim]
    scale = (2.0 ** rng.integers(-1, 2, obs_dim)).astype(np.float32)                  # 1/2, 1, 2
    sizes = (1, 63, 64, 65, 200)
    for attempt in range(50):     # redraw until the premise holds
        layers = [(sparse_signs(rng, dims[L], dims[L + 1], 6 if L == 0 else 2), rng.integers(-4, 5, dims[L + 1]).astype(np.float32) / 4)
                  for L in range(n_hidden + 1)]
        obs = {n: rng.integers(-8, 9, (n, obs_dim)).astype(np.float32) / 4 for n in sizes}
        want = {(n, s is not None): exact_chain(layers, obs[n], s, relu) for n in sizes for s in (None, scale)}
        if all(ok for _, ok in want.values()):
            break
    else:
        raise AssertionError('no draw satisfied the premise')
    act = 'relu' if relu else 'linear'
    for sc in (None, scale):
        m = f16_mlp(dev, obs_dim, n_hidden, n_units, out_dim, act, 'linear', layers, sc)
        for n in sizes:
            ref = want[(n, sc is not None)][0].astype(np.float32)
            assert np.array_equal(ref.astype(np.float64), want[(n, sc is not None)][0])
            assert same(mlp_f16_reference(layers, obs[n], act, 'linear', sc), ref)      # the restatement, fp32 sums in k order
            got = dev.mlp_forward(m, out_dim, obs[n])
            assert same(got, ref), 'n=%d scale=%s: %d of %d outputs differ, max |d| %.3g' % (
                n, sc is not None, int((got != ref).sum()), got.size, float(np.max(np.abs(got - ref))))
        dev.api.mlp_destroy(m)


# ---- 2: bound ----
def head(logits, action_range):
    mean = logits[:, :logits.shape[1] // 2]
    return (np.float32(action_range) * _tanh_det(mean)).astype(np.float32) if action_range > 0 else mean


@pytest.mark.parametrize('cfg', CONFIGS, ids=lambda c: '%dx%dx%d_%s' % (c[0], c[1], c[2], c[4]))
def test_random_networks_within_the_column_bound(cfg):
    """|got - ref64| <= 4 E_c + 2^-20 max|ref64| per output column, E_c = max over rows |ref32 - ref64| of the restatement's own two
    runs; every row counts.  Measured worst error / tolerance per config (MI355X): see DESIGN §15."""
    obs_dim, n_hidden, n_units, out_dim, hact, oact = cfg
    rng = np.random.default_rng(obs_dim * 7 + n_units)
    dev = DeviceModel('left')
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim)
    scale = rng.uniform(0.05, 1.0, obs_dim).astype(np.float32)
    obs = (rng.standard_normal((256, obs_dim)) * 3).astype(np.float32)
    ok = np.ones(len(obs), bool)
    worst, failures = 0.0, []

    def check(got, r32, r64, what):
        nonlocal worst
        E = np.abs(r32.astype(np.float64) - r64).max(0)
        ratio = float((np.abs(got.astype(np.float64) - r64).max(0) / column_tolerance(E, r64, ok)).max())
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            failures.append((what, ratio))

    for sc in (None, scale):
        m = f16_mlp(dev, obs_dim, n_hidden, n_units, out_dim, hact, oact, layers, sc)
        ref32 = mlp_f16_reference(layers, obs, hact, oact, sc)
        ref64 = mlp_f16_reference(layers, obs, hact, oact, sc, accumulate=np.float64)
        check(dev.mlp_forward(m, out_dim, obs), ref32, ref64, 'logits, scale %s' % (sc is not None))
        if out_dim % 2 == 0:
            for ar in (1.0, 0.5, -1.0):
                check(dev.policy_run_batch(m, out_dim // 2, obs, ar), head(ref32, ar), head(ref64, ar), 'head %g, scale %s' % (ar, sc is not None))
        dev.api.mlp_destroy(m)
    print('%s: worst error / tolerance %.3f' % (cfg, worst))
    assert not failures, failures


# ---- shared: a model, start states and a 2 x 256 policy ----
def shield_case(task, N, B=300, seed=21, mode='training'):
    host, dev = record_host(task, n_veh=N, mode=mode), DeviceModel(task, n_veh=N, mode=mode)
    inp = make_rollout_inputs(task, B, N, 5, seed=seed)
    trk = host.tracking_error(inp['ego'][:, 3], inp['ego'][:, 4], inp['ego'][:, 5], inp['ego'][:, 0], 0, ref_idx=inp['ref_idx'])
    obs0 = assemble_obs(inp['ego'], trk, inp['veh'])
    rng = np.random.default_rng(N)
    layers = make_layers(rng, host.D, 2, 256, 4)
    scale = rng.uniform(0.02, 0.2, host.D).astype(np.float32)
    return host, dev, inp, obs0, (host.D, 2, 256, 4, 'elu', 'linear', layers, scale)


# ---- 3: nothing else moved ----
def test_fp32_handles_keep_the_oracle_bits():
    host, dev, inp, obs0, net = shield_case('left', 8)
    mh = host.make_mlp(*net)
    never = dev.make_mlp(*net)
    back = dev.make_mlp(*net)
    dev.api.mlp_set_precision(back, F16)
    moved = dev.mlp_forward(back, 4, obs0)
    dev.api.mlp_set_precision(back, F32)
    want = host.mlp_forward(mh, 4, obs0)
    assert not same(moved, want)                                    # the switch does select another kernel
    for md in (never, back):
        assert same(dev.mlp_forward(md, 4, obs0), want)
        assert same(dev.policy_run_batch(md, 2, obs0, 1.0), host.policy_run_batch(mh, 2, obs0, 1.0))
        w = host.shield_is_safe(mh, obs0, ref_idx=inp['ref_idx'], steps=5, penalty=0)
        g = dev.shield_is_safe(md, obs0, ref_idx=inp['ref_idx'], steps=5, penalty=0)
        assert same(g[0], w[0]) and same(g[1], w[1]) and same(g[2], w[2]) and same(g[3], w[3])   # (penalty sums: the oracle in the kernels' order)
        dev.api.mlp_destroy(md)
    host.api.mlp_destroy(mh)


# ---- 4: properties ----
@pytest.mark.parametrize('dims,hact', [((16, 2, 64, 4), 'elu'), ((16, 2, 64, 4), 'tanh'), ((33, 4, 100, 6), 'relu'), ((137, 2, 256, 4), 'elu')],
                         ids=lambda v: v if isinstance(v, str) else '%dx%dx%dx%d' % v)
def test_rows_are_independent_and_launches_repeat(dims, hact):
    obs_dim, n_hidden, n_units, out_dim = dims
    rng = np.random.default_rng(obs_dim + n_units)
    dev = DeviceModel('left')
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim, bias_scale=1.0)
    m = f16_mlp(dev, obs_dim, n_hidden, n_units, out_dim, hact, 'linear', layers)
    obs = (rng.standard_normal((333, obs_dim)) * 2).astype(np.float32)
    first = dev.mlp_forward(m, out_dim, obs)
    assert same(dev.mlp_forward(m, out_dim, obs), first)                                     # a launch repeats its bits
    perm = rng.permutation(len(obs))
    assert same(dev.mlp_forward(m, out_dim, obs[perm]), first[perm])                         # position in the batch
    assert same(dev.mlp_forward(m, out_dim, obs[100:171]), first[100:171])                   # neighbours and n
    assert same(dev.policy_run_batch(m, out_dim // 2, obs[5:6], 1.0), dev.policy_run_batch(m, out_dim // 2, obs, 1.0)[5:6])
    # non-finite rows: the restatement's pattern, and every other row untouched
    bad = obs.copy()
    bad[:8, 3] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-38, -1e-38, 3e38]
    got, ref = dev.mlp_forward(m, out_dim, bad), mlp_f16_reference(layers, bad, hact, 'linear')
    assert same(np.isnan(got), np.isnan(ref)) and same(np.isinf(got), np.isinf(ref))
    assert same(np.sign(got[np.isinf(got)]), np.sign(ref[np.isinf(ref)]))
    assert same(got[8:], first[8:]) and np.all(np.isfinite(got[3:7]))
    # n = 0 is a no-op
    out = dev._out((4, out_dim))
    dev.api.mlp_forward(m, 0, None, None, dev.stream)
    dev.api.policy_run_batch(m, 0, None, C.c_float(1.0), dev._ptr(out), dev.stream)
    dev.api.mlp_destroy(m)


# ---- 5: shield ----
def generic_loop(dev, m, obs0, ref_idx, steps, penalty):
    view = loop_view(loop(dev, m, obs0, steps, ref_idx), steps, penalty)
    return view['safe'], view['punish'], view['last']


@pytest.mark.parametrize('task,N', [('left', 8), ('right', 5), ('left', 32)])
def test_shield_equals_the_generic_loop_bitwise(task, N):
    _host, dev, inp, obs0, net = shield_case(task, N)
    m = f16_mlp(dev, *net)
    for steps, penalty in ((5, 0), (20, 1)):
        safe, punish, last, _ = dev.shield_is_safe(m, obs0, ref_idx=inp['ref_idx'], steps=steps, penalty=penalty)
        want = generic_loop(dev, m, obs0, inp['ref_idx'], steps, penalty)
        for name, g, w in zip(('safe', 'punish', 'last obs'), (safe, punish, last), want):
            assert same(g, w), '%s differs (penalty %d, %d steps)' % (name, penalty, steps)
    dev.api.mlp_destroy(m)


# ---- 6: G14 ----
@pytest.mark.parametrize('name', G14)
def test_g14_safe_flags_with_the_fixture_weights_in_fp16(name):
    g = golden(name)
    task = name.split('_')[-1]
    n = len([k for k in g.files if k.startswith('policy_w')])
    layers = [(g['policy_w%d' % (2 * i)], g['policy_w%d' % (2 * i + 1)]) for i in range(n // 2)]
    dev = DeviceModel(task, mode='selecting')
    m = f16_mlp(dev, g['obs'].shape[1], n // 2 - 1, layers[0][0].shape[1], 4, 'elu', 'linear', layers, g['obs_scale'])
    safe, punish, _, _ = dev.shield_is_safe(m, g['obs'], ref_idx=None, path_id=int(g['path_index']), steps=5, penalty=0)
    assert np.array_equal(safe, g['safe']), 'safe flags differ from the reference at %s' % np.flatnonzero(safe != g['safe'])
    assert np.array_equal(punish > 0, g['safe'] == 0)
    dev.api.mlp_destroy(m)


# ---- 7: refusals ----
def test_precision_entries_refuse_bad_arguments():
    dev = DeviceModel('left')
    api = dev.api
    m = dev.make_mlp(8, 1, 64, 4, 'elu', 'linear', make_layers(np.random.default_rng(0), 8, 1, 64, 4))
    p = C.c_int32(-5)
    api.mlp_get_precision(m, C.byref(p))
    assert p.value == F32                                            # the default
    for bad in (2, -1, 99):
        with pytest.raises(ValueError, match='unknown precision'):
            api.mlp_set_precision(m, bad)
    api.mlp_get_precision(m, C.byref(p))
    assert p.value == F32                                            # a refused value leaves the handle as it was
    with pytest.raises(ValueError, match='null handle'):
        api.mlp_set_precision(None, F16)
    with pytest.raises(ValueError, match='null handle'):
        api.mlp_get_precision(None, C.byref(p))
    with pytest.raises(ValueError, match='null output pointer'):
        api.mlp_get_precision(m, None)
    for want in (F16, F32, F16):
        api.mlp_set_precision(m, want)
        api.mlp_get_precision(m, C.byref(p))
        assert p.value == want
    assert api.mlp_f16_fn('eb_mlp_f16_abi_version')() == _capi.EB_MLP_F16_ABI_VERSION == 1
    api.mlp_destroy(m)


# ---- 8: façade ----
def test_facade_precision_switch_and_native_shield():
    import torch
    from types import SimpleNamespace
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.policy import LoadPolicy, MLPNet
    from env_build_amd.shield import is_safe
    task, N, B = 'left', 8, 300
    model = EnvironmentModel(task, 0, mode='selecting', n_veh=N)
    D = model.obs_dim
    scale = [0.2] * 6 + [1., 1 / 30., 0.2] + [1 / 30., 1 / 30., 0.2, 1 / 180.] * N
    args = dict(obs_dim=D, act_dim=2, num_hidden_layers=2, num_hidden_units=256, hidden_activation='elu', policy_out_activation='linear',
                action_range=1.0, deterministic_policy=True, obs_preprocess_type='scale', obs_scale=scale)
    pol16 = LoadPolicy(args=SimpleNamespace(policy_precision='fp16', **args))
    pol32 = LoadPolicy(args=SimpleNamespace(**args))
    assert pol16.policy.policy.precision == pol16.policy.obj_v.precision == 'fp16' and pol32.policy.policy.precision == 'fp32'
    inp = make_rollout_inputs(task, B, N, 5, seed=2)
    host = HostModel(oracle_lib(), task, n_veh=N, mode='selecting')
    trk = host.tracking_error(inp['ego'][:, 3], inp['ego'][:, 4], inp['ego'][:, 5], inp['ego'][:, 0], 0, path_id=1)
    obs0 = assemble_obs(inp['ego'], trk, inp['veh'])
    # the façade's outputs are the C entries' bits
    dev = DeviceModel(task, n_veh=N, mode='selecting')
    w = pol16.policy.policy.get_weights()
    layers = list(zip(w[0::2], w[1::2]))
    m = f16_mlp(dev, D, 2, 256, 4, 'elu', 'linear', layers, np.asarray(scale, np.float32))
    want16 = dev.policy_run_batch(m, 2, obs0, 1.0)
    assert same(pol16.run_batch(obs0).numpy(), want16)
    assert same(pol16.policy.policy(obs0).numpy(), dev.mlp_forward(m, 4, obs0))
    assert not same(pol32.run_batch(obs0).numpy(), want16)          # same seed, same weights, the fp32 kernel
    # MLPNet(precision=...) and set_precision, surviving set_weights / set_obs_scale (which rebuild the handle)
    net = MLPNet(D, 2, 256, 'elu', 4, precision='fp16')
    net.set_weights(w)
    net.set_obs_scale(np.asarray(scale, np.float32))
    assert net.precision == 'fp16' and same(net.mode(obs0, 1.0).numpy(), want16)
    net.set_precision('fp32')
    assert same(net.mode(obs0, 1.0).numpy(), pol32.run_batch(obs0).numpy())
    net.set_precision('fp16')
    assert same(net.mode(obs0, 1.0).numpy(), want16)
    with pytest.raises(ValueError):
        net.set_precision('bf16')
    with pytest.raises(ValueError):
        MLPNet(D, 2, 256, 'elu', 4, precision='half')
    # shield.is_safe through the fp16 policy == test 5's loop through the C entries
    safe_n, pun_n = is_safe(model, pol16, obs0, path_index=1, steps=5)
    last_n = model.obses.numpy()
    obs, punish = obs0, None
    for _ in range(5):
        obs, out5, _ = dev.rollout_step(obs, dev.policy_run_batch(m, 2, obs, 1.0), None, path_id=1)
        punish = out5[3].copy() if punish is None else punish + out5[3]
    assert same(safe_n.numpy(), ~(punish > 0)) and same(pun_n.numpy(), punish) and same(last_n, obs)
    dev.api.mlp_destroy(m)
    torch.cuda.synchronize()
