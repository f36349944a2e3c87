"""GPU (-m gpu): the policy network's backward (env_build_amd/csrc/eb_policy_grad.hip, include/envbuild_mlp_grad.h) through the C-ABI and
the façade.  The backward sums take the kernels' own order, so the entry is held to (1) the bits of the float64 restatement where every
partial sum is exact, (2) a bound from the restatement's own float32 / float64 runs on random networks, (2b) the bits of the float32
restatement where every backward sum has one non-zero term at most, for every activation and head, (3) the forward's bits in `out`
and untouched forwards, (4) repeatability and row independence, (5) the device-side weight set against the host one bit for bit,
(6) clean refusals, (7) the façade and the example."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from env_build_amd import _capi  # noqa: E402
from env_build_amd import policy_grad  # noqa: E402
from env_build_amd.policy_grad import _act, mlp_backward_reference  # noqa: E402
from tests._helpers import DeviceModel, HostModel, oracle_lib  # noqa: E402
from tests._policy import F16, F32, SENTINEL, param_count, same, sparse_signs, split_params  # noqa: E402
from tests._policy_cases import make_layers, torch_twin  # noqa: E402

pytestmark = pytest.mark.gpu


def backward(dev, m, dims, obs, g, head=0, action_range=1.0, want=('out', 'g_obs', 'g_params')):
    """one eb_mlp_backward -> (out, g_obs, [g_params]) as NumPy (None where not asked for); outputs are pre-filled with SENTINEL"""
    api, torch = dev.api, dev.torch
    n = len(obs)
    ob, gg = dev._in(obs), dev._in(g)
    need = C.c_size_t(0)
    api.mlp_backward_workspace_bytes(m, n, C.byref(need))
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev.dev)
    cols = dims[3] if head == 0 else dims[3] // 2
    out = torch.full((n, cols), SENTINEL, device=dev.dev) if 'out' in want else None
    g_obs = torch.full((n, dims[0]), SENTINEL, device=dev.dev) if 'g_obs' in want else None
    g_par = torch.full((param_count(dev, m),), SENTINEL, device=dev.dev) if 'g_params' in want else None
    api.mlp_backward(m, n, dev._ptr(ob), dev._ptr(gg), head, C.c_float(action_range), dev._ptr(ws), need.value, dev._ptr(out),
                     dev._ptr(g_obs), dev._ptr(g_par), dev.stream)
    torch.cuda.synchronize()
    ret = lambda t: None if t is None else t.cpu().numpy()
    return ret(out), ret(g_obs), (None if g_par is None else split_params(ret(g_par), dims))


def empty_handle(dev, dims, hact, oact):
    """eb_mlp_create alone: no layer set"""
    cfg = _capi.EbMlpConfig(_capi.EB_ABI_VERSION, dims[0], dims[1], dims[2], dims[3], _capi.ACT_ID[hact], _capi.ACT_ID[oact], 0)
    m = C.c_void_p()
    dev.api.check(dev.api.lib.eb_mlp_create(C.byref(cfg), C.byref(m)))
    return m


def flat_of(layers):
    return np.concatenate([np.asarray(a, np.float32).ravel() for pair in layers for a in pair])


# ---- 1: exact ----
EXACT_SHAPES = [(9, 1, 64, 2), (29, 1, 64, 4), (41, 2, 256, 4), (137, 2, 256, 4), (45, 3, 128, 4), (33, 4, 100, 4), (8, 8, 32, 2),
                (137, 2, 200, 1), (137, 1, 64, 4),
                # out_dim 8 .. 32: the output layer's transposed product with 1 .. 4 steps, its second 16-column tile, head 1 with
                # act_dim 9 / 12 / 16; obs_dim 192 / 193 / 300: the second trip of the x_0 staging loop, 7 / 10 column tiles of g_obs
                (16, 2, 64, 8), (193, 2, 64, 9), (192, 1, 256, 16), (137, 1, 64, 17), (41, 2, 256, 18), (45, 3, 128, 24), (29, 1, 64, 32),
                (300, 1, 128, 4)]
EXACT_SIZES = (1, 63, 64, 65, 200, 1100)      # 1100 rows: three row splits of the parameter gradients (512, 512, 76)
# 2048: four full splits; 2049: a fifth split of one row in a second y block of mlp_wgrad_kernel, three idle waves; 4160: nine splits
# in three y blocks and 65 full row blocks.  One shape per width.
MANY_ROWS_SIZES = (2048, 2049, 4160)
MANY_ROWS_SHAPES = [(29, 1, 64, 32), (45, 3, 128, 24), (41, 2, 256, 4)]
EXACT_CASES = [(s, EXACT_SIZES) for s in EXACT_SHAPES] + [(s, MANY_ROWS_SIZES) for s in MANY_ROWS_SHAPES]
EXACT_IDS = ['%dx%dx%dx%d' % s for s in EXACT_SHAPES] + ['%dx%dx%dx%d-2048+' % s for s in MANY_ROWS_SHAPES]
GRAN = 2.0 ** -4


def exact_premise(layers, obs, g, scale, relu, head):
    """float64 (every value exact there): for the forward and all three backward products, sum |products| < 2^20 and every result a
    multiple of 2^-4 — then every partial sum, in ANY order, is an integer multiple of 2^-4 below 2^20 and fp32 sums are exact"""
    ok = True

    def product(a, b, bias=None):
        nonlocal ok
        mass = np.abs(a) @ np.abs(b) + (0.0 if bias is None else np.abs(bias))
        out = a @ b + (0.0 if bias is None else bias)
        ok = ok and bool(np.all(mass < 2.0 ** 20)) and bool(np.all(np.round(out / GRAN) == out / GRAN))
        return out

    f = lambda a: np.asarray(a, np.float64)
    sc = np.ones(obs.shape[1]) if scale is None else f(scale)
    xs = [f(obs) * sc]
    ok = ok and bool(np.all(np.round(xs[0] / GRAN) == xs[0] / GRAN))
    for L, (w, b) in enumerate(layers):
        pre = product(xs[-1], f(w), f(b))
        xs.append(np.maximum(pre, 0.0) if relu and L < len(layers) - 1 else pre)
    y = xs.pop()
    d = f(g) if head == 0 else np.concatenate([f(g), np.zeros((len(y), y.shape[1] - g.shape[1]))], 1)
    for L in range(len(layers) - 1, -1, -1):
        product(xs[L].T, d)
        product(np.ones((1, len(d))), d)
        d = product(d, f(layers[L][0]).T)
        if L > 0 and relu:
            d = d * (xs[L] > 0)
    return ok


@pytest.mark.parametrize('shape,sizes', EXACT_CASES, ids=EXACT_IDS)
def test_exact_inputs_give_the_restatement_bits(shape, sizes):
    obs_dim, n_hidden, n_units, out_dim = shape
    relu = EXACT_SHAPES.index(shape) % 2 == 0
    act = 'relu' if relu else 'linear'
    heads = (0, 1) if out_dim % 2 == 0 else (0,)
    rng = np.random.default_rng(obs_dim * 31 + n_units)
    dev = DeviceModel('left')
    dims = [obs_dim] + [n_units] * n_hidden + [out_dim]
    scale = (2.0 ** rng.integers(0, 2, obs_dim)).astype(np.float32)                   # 1, 2
    for attempt in range(20):     # redraw until the premise holds
        layers = [(sparse_signs(rng, dims[L], dims[L + 1], 6 if L == 0 else 3), rng.integers(-4, 5, dims[L + 1]).astype(np.float32) / 4)
                  for L in range(n_hidden + 1)]
        obs = {n: rng.integers(-8, 9, (n, obs_dim)).astype(np.float32) / 4 for n in sizes}
        g = {(n, h): rng.integers(-4, 5, (n, out_dim if h == 0 else out_dim // 2)).astype(np.float32) / 4 for n in sizes for h in heads}
        if all(exact_premise(layers, obs[n], g[(n, h)], sc, relu, h) for n in sizes for h in heads for sc in (None, scale)):
            break
    else:
        raise AssertionError('no draw satisfied the premise')
    for sc in (None, scale):
        m = dev.make_mlp(obs_dim, n_hidden, n_units, out_dim, act, 'linear', layers, sc)
        for n in sizes:
            for h in heads:
                want = mlp_backward_reference(layers, obs[n], g[(n, h)], act, 'linear', sc, h, -1.0, dtype=np.float64)
                got = backward(dev, m, shape, obs[n], g[(n, h)], h, -1.0)
                pairs = [('out', got[0], want[0]), ('g_obs', got[1], want[1])] + [('g_params[%d]' % k, a, b)
                                                                                 for k, (a, b) in enumerate(zip(got[2], want[2]))]
                for what, a, b in pairs:
                    assert a.dtype == np.float32 and np.array_equal(b.astype(np.float32).astype(np.float64), b), what
                    assert same(a, b.astype(np.float32)), '%s, n=%d head=%d scale=%s: %d of %d differ, max |d| %.3g' % (
                        what, n, h, sc is not None, int((a != b).sum()), a.size, float(np.max(np.abs(a - b))))
                assert n < 200 or (np.any(want[1] != 0) and np.any(want[2][0] != 0))         # the case says something
        dev.api.mlp_destroy(m)


# ---- 2: bound ----
RANDOM_CONFIGS = [(41, 2, 256, 4, 'elu', 'linear'), (137, 2, 256, 4, 'elu', 'linear'), (29, 1, 64, 4, 'relu', 'linear'),
                  (45, 3, 128, 4, 'relu', 'linear'), (45, 3, 128, 1, 'tanh', 'linear'), (33, 4, 100, 6, 'elu', 'tanh'),
                  (8, 8, 32, 2, 'tanh', 'linear'), (137, 2, 200, 4, 'relu', 'linear'), (17, 1, 1, 1, 'elu', 'linear')]
# the project's critic (a relu output); both tiles of the output layer with random weights; obs_dim 300 at width 256, elu output
WIDE_CONFIGS = [(45, 3, 100, 1, 'tanh', 'relu'), (29, 1, 64, 32, 'elu', 'linear'), (137, 2, 128, 17, 'relu', 'tanh'),
                (300, 1, 256, 18, 'elu', 'elu'), (41, 2, 128, 8, 'elu', 'linear')]
# 2049 rows: five row splits, the last of one row in a second y block (the float32 restatement loops over the rows in Python: two small ones)
MANY_ROWS_CONFIGS = [(29, 1, 64, 4, 'relu', 'linear'), (41, 2, 128, 8, 'elu', 'linear')]
RANDOM_CASES = [(c, 200) for c in RANDOM_CONFIGS + WIDE_CONFIGS] + [(c, 2049) for c in MANY_ROWS_CONFIGS]
RANDOM_IDS = ['%dx%dx%d_%s' % (c[0], c[1], c[2], c[4]) for c in RANDOM_CONFIGS] + \
             ['%dx%dx%dx%d_%s_%s' % c for c in WIDE_CONFIGS] + ['%dx%dx%dx%d_%s_%s-2049' % c for c in MANY_ROWS_CONFIGS]


def rows_off_the_relu_kink(layers, obs, scale, hact='relu', oact='linear'):
    """rows none of whose relu pre-activations (float64) lies within 2^-16 (|b| + sum |x w|) of zero: the hidden layers' when the hidden
    activation is relu, the output layer's when the output activation is"""
    x = obs.astype(np.float64) * (1.0 if scale is None else scale.astype(np.float64))
    keep = np.ones(len(obs), bool)
    for L, (w, b) in enumerate(layers):
        act = oact if L == len(layers) - 1 else hact
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        pre, mass = x @ w64 + b64, np.abs(x) @ np.abs(w64) + np.abs(b64)
        if act == 'relu':
            keep &= ~np.any(np.abs(pre) < 2.0 ** -16 * mass, 1)
        x = _act(act, pre, np.float64)
    return keep


def bound_check(got, r32, r64, what, failures):
    """out and g_obs per column, every parameter tensor as a whole: |got - ref64| <= 4 E + 2^-20 max |ref64|, E = max |ref32 - ref64|"""
    worst = 0.0
    tensors = [('out', got[0], r32[0], r64[0], 0), ('g_obs', got[1], r32[1], r64[1], 0)]
    tensors += [('g_params[%d]' % k, got[2][k], r32[2][k], r64[2][k], None) for k in range(len(r64[2]))]
    for name, a, b32, b64, axis in tensors:
        E = np.abs(b32.astype(np.float64) - b64).max(axis)
        tol = 4.0 * E + 2.0 ** -20 * np.abs(b64).max(axis)
        ratio = float((np.abs(a.astype(np.float64) - b64).max(axis) / np.maximum(tol, 1e-300)).max())
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            failures.append((what, name, ratio))
    return worst


@pytest.mark.parametrize('cfg,n', RANDOM_CASES, ids=RANDOM_IDS)
def test_random_networks_within_the_bound(cfg, n):
    """Measured worst error / tolerance per config (MI355X): see DESIGN §17."""
    obs_dim, n_hidden, n_units, out_dim, hact, oact = cfg
    dims = (obs_dim, n_hidden, n_units, out_dim)
    rng = np.random.default_rng(0)
    layers = make_layers(rng, obs_dim, n_hidden, n_units, out_dim)
    obs = rng.standard_normal((n, obs_dim)).astype(np.float32)
    scale = rng.uniform(0.25, 1.0, obs_dim).astype(np.float32)
    dev = DeviceModel('left')
    worst, failures = 0.0, []
    cases = [(0, 1.0)] + ([(1, 1.0), (1, 0.5), (1, -1.0)] if out_dim % 2 == 0 else [])
    for sc in (None, scale):
        rows = obs
        if 'relu' in (hact, oact):        # rows on a kink leave the batch BEFORE the kernel runs: the parameter sums cover the same rows
            keep = rows_off_the_relu_kink(layers, obs, sc, hact, oact)
            assert keep.sum() >= 0.9 * len(obs), 'more than 10 %% of the rows removed: %d' % int((~keep).sum())
            rows = obs[keep]
        m = dev.make_mlp(obs_dim, n_hidden, n_units, out_dim, hact, oact, layers, sc)
        for head, ar in cases:
            g = rng.standard_normal((len(rows), out_dim if head == 0 else out_dim // 2)).astype(np.float32)
            r32 = mlp_backward_reference(layers, rows, g, hact, oact, sc, head, ar, dtype=np.float32)
            r64 = mlp_backward_reference(layers, rows, g, hact, oact, sc, head, ar, dtype=np.float64)
            got = backward(dev, m, dims, rows, g, head, ar)
            worst = max(worst, bound_check(got, r32, r64, 'head %d range %g scale %s' % (head, ar, sc is not None), failures))
        dev.api.mlp_destroy(m)
    print('%s, %d rows: worst error / tolerance %.3f' % (cfg, n, worst))
    assert not failures, failures


def test_the_relu_rule_removes_what_the_issue_counted():
    """the rule itself, on the CPU side of this module: seed 0 removes 2 of 200 rows at 29x1x64 and 3 of 200 at 45x3x128; of the later
    configs, none of 200 at the critic's relu output (45x3x100 -> 1, tanh hidden), 2 of 200 at 137x2x128 -> 17 and 6 of 2049 at 29x1x64
    (with the scale on: 0, 5 and 7) — all far inside the 10 % cap"""
    for dims, hact, oact, n, n_removed, n_removed_scaled in (((29, 1, 64, 4), 'relu', 'linear', 200, 2, 0),
                                                             ((45, 3, 128, 4), 'relu', 'linear', 200, 3, 5),
                                                             ((45, 3, 100, 1), 'tanh', 'relu', 200, 0, 0),
                                                             ((137, 2, 128, 17), 'relu', 'tanh', 200, 2, 5),
                                                             ((29, 1, 64, 4), 'relu', 'linear', 2049, 6, 7)):
        rng = np.random.default_rng(0)
        layers = make_layers(rng, *dims)
        obs = rng.standard_normal((n, dims[0])).astype(np.float32)
        scale = rng.uniform(0.25, 1.0, dims[0]).astype(np.float32)
        if oact == 'linear':
            assert int((~rows_off_the_relu_kink(layers, obs, None)).sum()) == n_removed, dims       # the defaults: a relu / linear network
        assert int((~rows_off_the_relu_kink(layers, obs, None, hact, oact)).sum()) == n_removed, dims
        assert int((~rows_off_the_relu_kink(layers, obs, scale, hact, oact)).sum()) == n_removed_scaled, dims


# ---- 2b: one term per sum ----
ONE_TERM_SHAPES = [(41, 2, 64, 32), (137, 2, 256, 4), (45, 3, 100, 6)]
ONE_TERM_ROWS = (0, 63, 64, 511, 512, 599)       # of 600: the ends of a row block and of a row split
ONE_TERM_N = 600


def permutation_layers(rng, dims):
    """Kernels with at most one non-zero per row and per column, magnitudes in [0.5, 2], random signs, and random biases; every output
    column is tied back to an input through one unit per layer.  -> (layers, paths): paths[c] = the input and the units column c hangs on."""
    obs_dim, n_hidden, n_units, out_dim = dims
    d = [obs_dim] + [n_units] * n_hidden + [out_dim]
    assert out_dim <= obs_dim <= n_units
    value = lambda size: (rng.uniform(0.5, 2.0, size) * rng.choice([-1.0, 1.0], size)).astype(np.float32)
    layers, ends = [None] * (n_hidden + 1), np.arange(out_dim)           # ends: the column of layer L each path leaves through
    paths = [[c] for c in range(out_dim)]
    for L in range(n_hidden, -1, -1):
        k, cols = d[L], d[L + 1]
        m = min(k, cols)
        others = np.setdiff1d(np.arange(cols), ends)
        used_cols = np.concatenate([ends, rng.permutation(others)[:m - len(ends)]])
        keep = np.concatenate([np.ones(len(ends), bool), rng.random(m - len(ends)) < 0.9])       # partial: a tenth of the rest stays empty
        used_rows = rng.permutation(k)[:m]
        w = np.zeros((k, cols), np.float32)
        w[used_rows[keep], used_cols[keep]] = value(int(keep.sum()))
        layers[L] = (w, rng.uniform(-1.0, 1.0, cols).astype(np.float32))
        ends = used_rows[:len(ends)]
        for c in range(out_dim):
            paths[c].insert(0, int(ends[c]))
    return layers, paths


def path_is_live(layers, path, hact, oact, z, head_tanh):
    """float64, elementwise in z (the scaled input the path starts from): no relu on the path within 0.05 of its kink or below it, no
    tanh beyond 4 — the derivative along the path is then far from zero in float32 too"""
    ok = np.ones(z.shape, bool)
    for L, (w, b) in enumerate(layers):
        act = oact if L == len(layers) - 1 else hact
        pre = float(b[path[L + 1]]) + float(w[path[L], path[L + 1]]) * z
        ok &= (pre > 0.05) if act == 'relu' else (np.abs(pre) < 4.0) if act == 'tanh' else (pre > -4.0)
        z = _act(act, pre, np.float64)
    return ok & (np.abs(z) < 4.0 if head_tanh else True)


def one_term_case(rng, dims, hact, oact):
    """-> (layers, paths) in which every output column's path is live over a good part of the inputs: the biases on a path are redrawn
    until a twentieth of a standard normal sample passes path_is_live at scale 1 and at scale 1/4"""
    layers, paths = permutation_layers(rng, dims)
    z = rng.standard_normal(1024)
    for path in paths:
        for attempt in range(2000):
            if all(path_is_live(layers, path, hact, oact, z * s, True).mean() >= 0.05 for s in (1.0, 0.25)):
                break
            for L in range(len(layers)):
                layers[L][1][path[L + 1]] = rng.uniform(-1.0, 1.0)
        else:
            raise AssertionError('no biases keep the path of a column alive')
    return layers, paths


def one_term_inputs(rng, layers, paths, hact, oact, scale, gcols, head_tanh, turn):
    """obs and g_out of ONE_TERM_N rows: min(gcols, n) live rows, ONE_TERM_ROWS first (rotated by `turn`), each with one non-zero cotangent in
    a column of its own and with the input its path starts from drawn until path_is_live"""
    n, obs_dim = ONE_TERM_N, layers[0][0].shape[0]
    obs = rng.standard_normal((n, obs_dim)).astype(np.float32)
    first = list(np.roll(ONE_TERM_ROWS, -turn))
    rest = rng.permutation(np.setdiff1d(np.arange(n), ONE_TERM_ROWS))
    rows = np.array(first + list(rest))[:gcols]
    cols = rng.permutation(gcols)
    g = np.zeros((n, gcols), np.float32)
    for r, c in zip(rows, cols):
        k = paths[c][0]
        sc = 1.0 if scale is None else float(scale[k])
        draws = rng.standard_normal(4096).astype(np.float32)
        live = path_is_live(layers, paths[c], hact, oact, draws.astype(np.float64) * sc, head_tanh)
        assert live.any(), (r, c)
        obs[r, k] = draws[np.argmax(live)]
        g[r, c] = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
    return obs, g, rows


def one_term_reference(layers, obs, g, hact, oact, scale, head, ar):
    """mlp_backward_reference in float32, with the premise asserted on every backward product it forms (those without a start): no sum of
    non-zero terms has more than one — so the float32 restatement is the kernel's bits whatever the kernel's order"""
    inner, products = policy_grad._product, []

    def watched(a, b, dtype, start=None):
        if start is None:         # ((a != 0) @ (b != 0)).max(): a column of b with one non-zero gives one term at most, the others are counted
            per_col = np.count_nonzero(b, 0)
            many = (a != 0).astype(np.int64) @ (b[:, per_col > 1] != 0).astype(np.int64)
            products.append(max(int(per_col.clip(0, 1).max()), int(many.max()) if many.size else 0))
        return inner(a, b, dtype, start)

    policy_grad._product = watched
    try:
        ref = mlp_backward_reference(layers, obs, g, hact, oact, scale, head, ar, dtype=np.float32)
    finally:
        policy_grad._product = inner
    assert len(products) == 3 * len(layers) and max(products) <= 1, products
    return ref


@pytest.mark.parametrize('oact', ['linear', 'tanh', 'relu', 'elu'])
@pytest.mark.parametrize('hact', ['elu', 'tanh', 'relu'])
@pytest.mark.parametrize('shape', ONE_TERM_SHAPES, ids=lambda s: '%dx%dx%dx%d' % s)
def test_one_term_per_sum_gives_the_restatement_bits(shape, hact, oact):
    """Every activation's derivative, the tanh head, action_range and the output activation's derivative held to bits: each backward sum
    has at most one non-zero term, adding zeros is exact, so the order of the kernels' sums does not matter."""
    obs_dim, n_hidden, n_units, out_dim = shape
    rng = np.random.default_rng(1000 * ONE_TERM_SHAPES.index(shape) + 10 * len(hact) + len(oact) + obs_dim)
    dev = DeviceModel('left')
    scale = rng.uniform(0.25, 1.0, obs_dim).astype(np.float32)
    layers, paths = one_term_case(rng, shape, hact, oact)
    handles = {False: dev.make_mlp(obs_dim, n_hidden, n_units, out_dim, hact, oact, layers, None),
               True: dev.make_mlp(obs_dim, n_hidden, n_units, out_dim, hact, oact, layers, scale)}
    turn = 0
    # action_range 0.3: multiplying by 1.0 or 0.5 is exact, so only a range that is no power of two pins the grouping (g * range) * (1 - t * t)
    for head, ar, scaled in [(h, r, sc) for sc in (False, True) for h, r in ((0, 1.0), (1, 1.0), (1, 0.5), (1, 0.3), (1, -1.0))]:
        m, sc = handles[scaled], scale if scaled else None
        gcols = out_dim if head == 0 else out_dim // 2
        obs, g, rows = one_term_inputs(rng, layers, paths, hact, oact, sc, gcols, head == 1 and ar > 0, turn)
        turn += gcols
        want = one_term_reference(layers, obs, g, hact, oact, sc, head, ar)
        got = backward(dev, m, shape, obs, g, head, ar)
        what = '%s -> %s, head %d range %g scale %s' % (hact, oact, head, ar, scaled)
        forward = dev.mlp_forward(m, out_dim, obs) if head == 0 else dev.policy_run_batch(m, gcols, obs, ar)
        assert same(got[0], forward), 'out, ' + what
        assert same(got[1], want[1]), 'g_obs, %s: %d of %d differ' % (what, int((got[1] != want[1]).sum()), want[1].size)
        for k, (a, b) in enumerate(zip(got[2], want[2])):
            assert same(a, b), 'g_params[%d], %s: %d of %d differ' % (k, what, int((a != b).sum()), b.size)
        # the case says something: every live row reaches the observations and no other does, every kernel has a gradient
        assert np.all(np.any(want[1][rows] != 0, 1)) and not np.any(np.delete(want[1], rows, 0)), what
        assert all(np.any(want[2][2 * L] != 0) for L in range(n_hidden + 1)), what
    for m in handles.values():
        dev.api.mlp_destroy(m)


# ---- shared by 3, 4: a random elu network ----
def elu_case(dims=(137, 2, 256, 4), n=200, seed=3):
    rng = np.random.default_rng(seed)
    layers = make_layers(rng, *dims, bias_scale=0.5)
    scale = rng.uniform(0.25, 1.0, dims[0]).astype(np.float32)
    obs = rng.standard_normal((n, dims[0])).astype(np.float32)
    return rng, layers, scale, obs


# ---- 3: the forward's bits ----
def test_out_is_the_forward_and_untouched_handles_keep_their_bits():
    dims = (137, 2, 256, 4)
    rng, layers, scale, obs = elu_case(dims)
    host, dev = HostModel(oracle_lib(), 'left'), DeviceModel('left')
    net = dims + ('elu', 'linear', layers, scale)
    mh, used, never = host.make_mlp(*net), dev.make_mlp(*net), dev.make_mlp(*net)
    logits = dev.mlp_forward(used, 4, obs)
    assert same(backward(dev, used, dims, obs, rng.standard_normal((200, 4)).astype(np.float32), 0)[0], logits)
    for ar in (1.0, 0.5, -1.0):
        got = backward(dev, used, dims, obs, rng.standard_normal((200, 2)).astype(np.float32), 1, ar)[0]
        assert same(got, dev.policy_run_batch(used, 2, obs, ar)), ar
    # fp32 is the oracle's chain, and a handle that has run the backward evaluates like one that never did, at either precision
    assert same(logits, host.mlp_forward(mh, 4, obs))
    for precision in (F32, F16, F32):
        for md in (used, never):
            dev.api.mlp_set_precision(md, precision)
        assert same(dev.mlp_forward(used, 4, obs), dev.mlp_forward(never, 4, obs))
        assert same(dev.policy_run_batch(used, 2, obs, 1.0), dev.policy_run_batch(never, 2, obs, 1.0))
    assert same(dev.mlp_forward(never, 4, obs), logits)
    for md in (used, never):
        dev.api.mlp_destroy(md)
    host.api.mlp_destroy(mh)


# ---- 4: rows ----
@pytest.mark.parametrize('dims,hact', [((16, 2, 64, 4), 'tanh'), ((33, 4, 100, 6), 'relu'), ((137, 2, 256, 4), 'elu')],
                         ids=lambda v: v if isinstance(v, str) else '%dx%dx%dx%d' % v)
def test_calls_repeat_and_rows_are_independent(dims, hact):
    rng, layers, scale, obs = elu_case(dims, n=333)
    dev = DeviceModel('left')
    m = dev.make_mlp(*dims, hact, 'linear', layers, scale)
    g = rng.standard_normal((333, dims[3])).astype(np.float32)
    first = backward(dev, m, dims, obs, g)
    again = backward(dev, m, dims, obs, g)
    assert same(again[0], first[0]) and same(again[1], first[1]) and all(same(a, b) for a, b in zip(again[2], first[2]))
    perm = rng.permutation(333)
    moved = backward(dev, m, dims, obs[perm], g[perm])
    assert same(moved[0], first[0][perm]) and same(moved[1], first[1][perm])
    part = backward(dev, m, dims, obs[100:171], g[100:171])
    assert same(part[0], first[0][100:171]) and same(part[1], first[1][100:171])
    only_obs = backward(dev, m, dims, obs, g, want=('g_obs',))
    assert only_obs[0] is None and only_obs[2] is None and same(only_obs[1], first[1])
    only_par = backward(dev, m, dims, obs, g, want=('g_params',))
    assert only_par[0] is None and only_par[1] is None and all(same(a, b) for a, b in zip(only_par[2], first[2]))
    # a non-finite row: every other row keeps its bits; where the activation passes NaN on (elu: inf times a padded unit's zero weight)
    # it poisons its own g_obs row and the parameter sums — relu turns NaN into 0 and a saturated tanh has derivative 0
    bad = obs.copy()
    bad[7, 3] = np.inf
    hit = backward(dev, m, dims, bad, g)
    keep = np.arange(333) != 7
    assert same(hit[0][keep], first[0][keep]) and same(hit[1][keep], first[1][keep])
    if hact == 'elu':
        assert not np.any(np.isfinite(hit[0][7])) and not np.any(np.isfinite(hit[1][7])) and not np.all(np.isfinite(hit[2][0]))
    # n = 0: g_params is written as zeros, nothing else is touched
    none = backward(dev, m, dims, obs[:0], g[:0])
    assert none[0].shape == (0, dims[3]) and all(np.all(t == 0) for t in none[2])
    torch = dev.torch
    g_par = torch.full((param_count(dev, m),), SENTINEL, device=dev.dev)
    dev.api.mlp_backward(m, 0, None, None, 0, C.c_float(1.0), None, 0, None, None, dev._ptr(g_par), dev.stream)
    dev.api.mlp_backward(m, 0, None, None, 0, C.c_float(1.0), None, 0, None, None, None, dev.stream)
    torch.cuda.synchronize()
    assert np.all(g_par.cpu().numpy() == 0)
    dev.api.mlp_destroy(m)


# ---- 5: device-side weight set ----
def special_values(with_inf):
    v = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2049.0, 2051.0,          # binary16 ties, up and down to even
         2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, -(2.0 ** -25), -1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25,   # subnormals
         65519.0, 65520.0, -65520.0, 65504.0, 0.0, -0.0]
    return np.array(v + ([np.inf, -np.inf] if with_inf else []), np.float32)


@pytest.mark.parametrize('dims', [(29, 1, 64, 4), (137, 2, 200, 6), (41, 2, 256, 4), (33, 3, 100, 32), (265, 2, 512, 4)],
                         ids=lambda s: '%dx%dx%dx%d' % s)
@pytest.mark.parametrize('with_inf', [False, True], ids=['finite', 'inf'])
def test_device_side_weight_set_equals_the_host_one(dims, with_inf):
    rng = np.random.default_rng(dims[0] + dims[2])
    layers = make_layers(rng, *dims, bias_scale=0.5)
    special = special_values(with_inf)
    for w, b in layers:           # the special values at random places of every kernel, and a few in the biases
        at = rng.choice(w.size, size=3 * len(special), replace=False)
        w.ravel()[at] = np.tile(special, 3)
        b[rng.choice(b.size, size=min(2, b.size), replace=False)] = special[[5, 16][:min(2, b.size)]]
    scale = rng.uniform(0.25, 1.0, dims[0]).astype(np.float32)
    obs = rng.standard_normal((130, dims[0])).astype(np.float32)
    obs[:, ::7] = 0.0
    dev = DeviceModel('left')
    torch = dev.torch
    host_built = dev.make_mlp(*dims, 'elu', 'linear', layers, scale)
    m = empty_handle(dev, dims, 'elu', 'linear')
    sc = np.ascontiguousarray(scale)
    dev.api.mlp_set_obs_scale(m, sc.ctypes.data)
    with pytest.raises(_capi.EbError, match='every layer'):
        dev.mlp_forward(m, dims[3], obs)
    flat = torch.from_numpy(flat_of(layers)).to(dev.dev)
    assert param_count(dev, m) == flat.numel()
    dev.api.mlp_set_params_device(m, dev._ptr(flat), dev.stream)
    for precision in (F32, F16):
        for md in (host_built, m):
            dev.api.mlp_set_precision(md, precision)
        a, b = dev.mlp_forward(m, dims[3], obs), dev.mlp_forward(host_built, dims[3], obs)
        assert same(a, b), 'precision %d: %d of %d logits differ' % (precision, int((a != b).sum()), a.size)
        assert same(dev.policy_run_batch(m, dims[3] // 2, obs, 1.0), dev.policy_run_batch(host_built, dims[3] // 2, obs, 1.0))
        assert with_inf or precision == F16 or np.all(np.isfinite(a))      # (65520 is inf in binary16)
    if dims[2] <= 256:
        for md in (host_built, m):
            dev.api.mlp_set_precision(md, F32)
        g = rng.standard_normal((130, dims[3])).astype(np.float32)
        a, b = backward(dev, m, dims, obs, g), backward(dev, host_built, dims, obs, g)
        assert same(a[0], b[0]) and same(a[1], b[1]) and all(same(x, y) for x, y in zip(a[2], b[2]))
    # a second set overwrites the first: the handle follows the buffer's new contents
    layers2 = make_layers(rng, *dims)
    flat.copy_(torch.from_numpy(flat_of(layers2)))
    dev.api.mlp_set_params_device(m, dev._ptr(flat), dev.stream)
    fresh = dev.make_mlp(*dims, 'elu', 'linear', layers2, scale)
    for precision in (F16, F32):
        for md in (fresh, m):
            dev.api.mlp_set_precision(md, precision)
        assert same(dev.mlp_forward(m, dims[3], obs), dev.mlp_forward(fresh, dims[3], obs))
    for md in (host_built, m, fresh):
        dev.api.mlp_destroy(md)


# ---- 6: refusals ----
def test_refusals_write_nothing():
    dev = DeviceModel('left')
    api, torch = dev.api, dev.torch
    rng = np.random.default_rng(0)
    dims = (8, 1, 64, 4)
    layers = make_layers(rng, *dims)
    obs, g = rng.standard_normal((10, 8)).astype(np.float32), rng.standard_normal((10, 4)).astype(np.float32)
    ob, gg = dev._in(obs), dev._in(g)
    ws = torch.empty((1 << 22,), dtype=torch.uint8, device=dev.dev)
    outs = [torch.full(s, SENTINEL, device=dev.dev) for s in ((10, 4), (10, 8), (8 * 64 + 64 + 64 * 4 + 4,))]

    def call(m, n=10, obs_p=ob, g_p=gg, head=0, ws_p=ws, ws_bytes=1 << 22):
        api.mlp_backward(m, n, dev._ptr(obs_p), dev._ptr(g_p), head, C.c_float(1.0), dev._ptr(ws_p), ws_bytes, *[dev._ptr(t) for t in outs],
                         dev.stream)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in outs)

    m = dev.make_mlp(*dims, 'elu', 'linear', layers)
    ok, need = C.c_int32(-1), C.c_size_t(0)
    api.mlp_grad_supported(m, C.byref(ok))
    assert ok.value == 1 and api.mlp_grad_fn('eb_mlp_grad_abi_version')() == _capi.EB_MLP_GRAD_ABI_VERSION == 1
    api.mlp_backward_workspace_bytes(m, 10, C.byref(need))
    assert 0 < need.value <= 1 << 22
    # fp16: refused on purpose, with the reason eb_mlp_grad_supported reports
    api.mlp_set_precision(m, F16)
    api.mlp_grad_supported(m, C.byref(ok))
    assert ok.value == 0 and b'EB_MLP_PRECISION_F32' in api.lib.eb_last_error()
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        call(m)
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        api.mlp_backward_workspace_bytes(m, 10, C.byref(need))
    api.mlp_set_precision(m, F32)
    # a workspace one byte short, head 1 with an odd out_dim (below), null pointers, bad n and head
    with pytest.raises(ValueError, match='workspace'):
        call(m, ws_bytes=need.value - 1)
    for kw in (dict(obs_p=None), dict(g_p=None), dict(ws_p=None)):
        with pytest.raises(ValueError, match='null obs, g_out or workspace'):
            call(m, **kw)
    with pytest.raises(ValueError, match='n < 0'):
        call(m, n=-1)
    with pytest.raises(ValueError, match='head must be'):
        call(m, head=2)
    with pytest.raises(ValueError, match='null handle'):
        call(None)
    for fn, args in ((api.mlp_grad_supported, (m, None)), (api.mlp_param_count, (m, None)), (api.mlp_backward_workspace_bytes, (m, 10, None))):
        with pytest.raises(ValueError, match='null output pointer'):
            fn(*args)
    with pytest.raises(ValueError, match='null params'):
        api.mlp_set_params_device(m, None, dev.stream)
    assert untouched()
    call(m, ws_bytes=need.value)                                      # and the exact size is enough
    assert not untouched()
    for t in outs:
        t.fill_(SENTINEL)
    api.mlp_destroy(m)
    odd = dev.make_mlp(8, 1, 64, 3, 'elu', 'linear', make_layers(rng, 8, 1, 64, 3))
    with pytest.raises(ValueError, match='out_dim = 2 \\* act_dim'):
        call(odd, head=1)
    api.mlp_destroy(odd)
    # width 300 pads to 512
    wide = dev.make_mlp(8, 1, 300, 4, 'elu', 'linear', make_layers(rng, 8, 1, 300, 4))
    api.mlp_grad_supported(wide, C.byref(ok))
    assert ok.value == 0 and b'pads to 512' in api.lib.eb_last_error()
    with pytest.raises(ValueError, match='pads to 512'):
        call(wide)
    api.mlp_destroy(wide)
    # a layer never set: EB_ESTATE
    unset = empty_handle(dev, dims, 'elu', 'linear')
    k, b = np.ascontiguousarray(layers[0][0]), np.ascontiguousarray(layers[0][1])
    api.mlp_set_layer(unset, 0, k.ctypes.data, b.ctypes.data)
    api.mlp_grad_supported(unset, C.byref(ok))
    assert ok.value == 0
    with pytest.raises(_capi.EbError, match='error -2.*never set'):
        call(unset)
    api.mlp_destroy(unset)
    assert untouched()


# ---- 7: façade ----
def test_trainable_mlpnet_gradients_optimiser_step_and_fp16():
    import torch
    from env_build_amd.policy import MLPNet
    from env_build_amd.policy_grad import TrainableMLPNet
    dims = (41, 2, 100, 4)
    rng = np.random.default_rng(11)
    net = TrainableMLPNet(dims[0], dims[1], dims[2], 'elu', dims[3], seed=4)
    assert isinstance(net, MLPNet)
    layers = make_layers(rng, *dims, bias_scale=0.3)
    net.set_weights([a for pair in layers for a in pair])
    scale = rng.uniform(0.25, 1.0, dims[0]).astype(np.float32)
    net.set_obs_scale(scale)
    params = net.parameters()
    assert len(params) == 6 and all(p.is_leaf and p.requires_grad and p.is_cuda for p in params)
    assert [tuple(p.shape) for p in params] == [a.shape for pair in layers for a in pair]
    assert all(p.untyped_storage().data_ptr() == params[0].untyped_storage().data_ptr() for p in params)   # views of ONE tensor
    assert all(np.array_equal(a, b) for a, b in zip(net.get_weights(), [a for pair in layers for a in pair]))
    obs = rng.standard_normal((200, dims[0])).astype(np.float32)
    failures = []
    for head, ar, cols in ((0, 1.0, 4), (1, 1.0, 2), (1, 0.5, 2)):
        g = rng.standard_normal((200, cols)).astype(np.float32)
        x = torch.from_numpy(obs).cuda().requires_grad_(True)
        for p in params:
            p.grad = None
        out = net.call(x) if head == 0 else net.mode(x, ar)
        assert isinstance(out, torch.Tensor) and out.requires_grad
        (out * torch.from_numpy(g).cuda()).sum().backward()
        got = (out.detach().cpu().numpy(), x.grad.cpu().numpy(), [p.grad.cpu().numpy() for p in params])
        want = torch_twin(layers, obs, g, 'elu', 'linear', scale, head, ar)
        r32 = mlp_backward_reference(layers, obs, g, 'elu', 'linear', scale, head, ar, dtype=np.float32)
        bound_check(got, r32, want, 'head %d range %g' % (head, ar), failures)
    assert not failures, failures
    # one optimiser step, no explicit sync: the next forward is a fresh MLPNet built from get_weights(), bit for bit
    opt = torch.optim.Adam(params, lr=1e-2)
    before = net.get_weights()
    opt.step()
    after = net.get_weights()
    assert all(np.any(a != b) for a, b in zip(before, after))
    fresh = MLPNet(dims[0], dims[1], dims[2], 'elu', dims[3])
    fresh.set_weights(after)
    fresh.set_obs_scale(scale)
    with torch.no_grad():
        assert same(net.call(obs).cpu().numpy(), fresh.call(obs).numpy())
        assert same(net.mode(obs, 1.0).cpu().numpy(), fresh.mode(obs, 1.0).numpy())
    # a backward whose weights changed since its forward raises
    out = net.call(obs)
    opt.step()
    with pytest.raises(RuntimeError, match='modified in place'):
        out.sum().backward()
    # fp16: inference on the same handle, differentiation refused with the C reason
    net.set_precision('fp16')
    fresh.set_weights(net.get_weights())
    fresh.set_precision('fp16')
    out16 = net.call(obs)
    assert same(out16.detach().cpu().numpy(), fresh.call(obs).numpy())
    with pytest.raises(ValueError, match='EB_MLP_PRECISION_F32'):
        out16.sum().backward()
    net.set_precision('fp32')
    net.call(obs).sum().backward()
    torch.cuda.synchronize()


def test_trainable_mlpnet_critic_with_a_relu_output():
    """the project's critic, MLPNet(D, 3, 100, 'tanh', 1, output_activation='relu'), as an ADP trainer differentiates it:
    call(x).sum().backward() against the torch twin under the rule of (2), rows on the output's kink leaving first"""
    import torch
    from env_build_amd.policy_grad import TrainableMLPNet
    dims = (41, 3, 100, 1)
    rng = np.random.default_rng(12)
    net = TrainableMLPNet(dims[0], dims[1], dims[2], 'tanh', dims[3], name='obj_v', output_activation='relu', seed=5)
    layers = make_layers(rng, *dims, bias_scale=0.3)
    net.set_weights([a for pair in layers for a in pair])
    scale = rng.uniform(0.25, 1.0, dims[0]).astype(np.float32)
    net.set_obs_scale(scale)
    params = net.parameters()
    obs = rng.standard_normal((200, dims[0])).astype(np.float32)
    keep = rows_off_the_relu_kink(layers, obs, scale, 'tanh', 'relu')
    assert keep.sum() >= 0.9 * len(obs)
    obs = obs[keep]
    x = torch.from_numpy(obs).cuda().requires_grad_(True)
    out = net.call(x)
    out.sum().backward()
    got = (out.detach().cpu().numpy(), x.grad.cpu().numpy(), [p.grad.cpu().numpy() for p in params])
    g = np.ones((len(obs), 1), np.float32)
    want = torch_twin(layers, obs, g, 'tanh', 'relu', scale, 0, 1.0)
    r32 = mlp_backward_reference(layers, obs, g, 'tanh', 'relu', scale, 0, 1.0, dtype=np.float32)
    failures = []
    worst = bound_check(got, r32, want, 'critic', failures)
    print('critic façade: worst error / tolerance %.3f' % worst)
    assert not failures, failures
    # both sides of the kink are in the batch, and the rows below it give exact zeros
    dead = want[0][:, 0] == 0
    assert dead.sum() >= 10 and (~dead).sum() >= 10 and not np.any(got[1][dead]) and np.all(np.any(got[1][~dead] != 0, 1))
    assert all(np.any(t != 0) for t in got[2])


def test_example_trains_the_project_network_and_rolls_it_out_in_fp16():
    import importlib.util
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.policy import MLPNet
    from env_build_amd.policy_rollout import policy_rollout
    spec = importlib.util.spec_from_file_location('adp_train_mlpnet', os.path.join(ROOT, 'examples', 'adp_train_mlpnet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.run(n_env=96, horizon=5, iterations=3)
    assert len(r['losses']) == 3 and np.all(np.isfinite(r['losses'])) and np.isfinite(r['grad_norm']) and r['grad_norm'] > 0
    assert all(bool((g != 0).any()) and bool(torch.isfinite(g).all()) for g in r['grads'])
    assert all(np.any(a != b) for a, b in zip(r['before'], r['after']))
    assert r['rollout']['fused'] is True
    # the same look-ahead from a host-built fp16 MLPNet(get_weights())
    net = r['policy']
    host_built = MLPNet(net.input_dim, net.num_hidden_layers, net.num_hidden_units, net.hidden_activation, 4, precision='fp16')
    host_built.set_weights(r['after'])
    host_built.set_obs_scale(mod.obs_scale(net.input_dim))
    model = EnvironmentModel(r['task'], mode='training', n_veh=r['n_veh'])
    model.reset(r['obs0'], r['ref_idx'])
    want = policy_rollout(model, mod.as_policy4toyota(host_built), r['obs0'], r['lookahead'], want=('out5', 'actions'))
    assert want['fused'] is True
    for key in ('obs', 'punish', 'safe', 'out5_steps', 'actions_steps'):
        assert same(r['rollout'][key].numpy(), want[key].numpy()), key
