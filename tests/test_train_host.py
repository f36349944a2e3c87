"""CPU (-m "not gpu"): the training family (include/envbuild_train.h, env_build_amd.train) — its header against the module's own binding
table and argument structs, the separation of libenvbuild_train.so from libenvbuild_hip.so and the kernels its code object holds,
device-free refusals, `adam_reference` in float64 against torch's float64 optimisers and in float32 under the 4 E rule, and
`value_loss_reference` against torch float64 autograd of the clipped value loss."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import train
from tests import _kernel_census as K
from tests._helpers import ROOT
from tests._ppo import within

HEADER = os.path.join(ROOT, 'include', 'envbuild_train.h')
KERNELS = ('adam_norm_kernel', 'adam_update_kernel', 'value_loss_kernel')        # DESIGN.md §24's list


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def ctype_of(decl, nested):
    decl = decl.replace('const ', '').strip()
    if decl.endswith('*'):
        return C.c_void_p
    if decl in nested:
        return nested[decl]
    return {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'float': C.c_float, 'double': C.c_double}[decl]


def struct_fields(src, name, nested=()):
    nested = dict(nested)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        if not decl.strip():
            continue
        first, *more = [p.strip() for p in decl.split(',')]
        m = re.match(r'(.*?)(\w+)(\[(\w+)\])?$', first)
        kind = ctype_of(m.group(1), nested)
        if m.group(4):
            kind = kind * {'EB_TRAIN_MAX_SEGMENTS': train.EB_TRAIN_MAX_SEGMENTS}[m.group(4)]
        fields.append((m.group(2), kind))
        fields += [(p, kind) for p in more]
    return fields


def test_header_declares_what_the_module_binds():
    text = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(train.TRAIN_PROTOTYPES) == ['eb_adam_step', 'eb_train_abi_version', 'eb_train_last_error', 'eb_value_loss']
    kinds = {'const eb_value_loss_args*': C.POINTER(train.EbValueLossArgs), 'const eb_adam_args*': C.POINTER(train.EbAdamArgs)}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, args) in train.TRAIN_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    assert not [n for n in names if re.search(r'_gate(d|_|$)', n)]
    for macro, value in (('EB_TRAIN_ABI_VERSION', train.EB_TRAIN_ABI_VERSION), ('EB_TRAIN_MAX_SEGMENTS', train.EB_TRAIN_MAX_SEGMENTS),
                         ('EB_TRAIN_ADAM_PARTIALS', train.EB_TRAIN_ADAM_PARTIALS)):
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert (train.EB_TRAIN_ABI_VERSION, train.EB_TRAIN_MAX_SEGMENTS) == (1, 32)
    assert struct_fields(src, 'eb_value_loss_args') == list(train.EbValueLossArgs._fields_)
    assert struct_fields(src, 'eb_adam_segment') == list(train.EbAdamSegment._fields_)
    assert struct_fields(src, 'eb_adam_state') == list(train.EbAdamState._fields_)
    assert struct_fields(src, 'eb_adam_args', {'eb_adam_segment': train.EbAdamSegment}) == list(train.EbAdamArgs._fields_)
    assert C.sizeof(train.EbAdamState) == 32 and C.sizeof(train.EbAdamSegment) == 40
    for struct in (train.EbValueLossArgs, train.EbAdamArgs):
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    for words in ('bit for bit', 'AT CALL TIME', 'tests/test_stream_census.py', 'ALWAYS exactly TWO launches', 'pure function of the counts',
                  'HALF', 'stay off it', 'a zero-filled state is a valid start', '4-byte alignment only', 'adam_reference',
                  'value_loss_reference', 'libenvbuild_train.so ONLY', 'takes the NEXT optimiser step', 'eb_train_last_error'):
        assert words in text, words


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import ppo
    assert not set(train.TRAIN_PROTOTYPES) & (set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES))
    for row in _capi.FAMILIES.values():
        assert not set(train.TRAIN_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in train.__all__]


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_train_sources_are_in_no_list_of_the_main_library():
    mine = {'eb_train.hip', 'eb_train.h', 'eb_train_device.h', os.path.join('..', '..', 'include', 'envbuild_train.h')}
    assert set(eb_build.TRAIN_SOURCES) == {'eb_train.hip'} and mine <= set(eb_build.TRAIN_SOURCES + eb_build.TRAIN_HEADERS)
    lists = [eb_build.SOURCES, eb_build.HEADERS] + list(eb_build.KERNEL_SOURCES.values())
    for files in lists:
        assert not [f for f in files if 'train' in f], files
    assert eb_build.TRAIN_LIB != eb_build.LIB and os.path.dirname(eb_build.TRAIN_LIB) == os.path.dirname(eb_build.LIB)
    assert os.path.basename(eb_build.TRAIN_LIB) == 'libenvbuild_train.so'
    assert eb_build.train_source_hash() != eb_build.source_hash()
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in ('eb_train.hip', 'eb_train.h', 'eb_train_device.h'))
    included = set(re.findall(r'#include "([^"]+)"', unit))
    assert {os.path.normpath(f) for f in included} <= {os.path.normpath(f) for f in eb_build.TRAIN_SOURCES + eb_build.TRAIN_HEADERS}
    # no unit of the main library includes a training header
    for f in eb_build.SOURCES + eb_build.HEADERS:
        assert 'eb_train' not in open(os.path.join(eb_build.CSRC, f)).read() and 'envbuild_train' not in open(os.path.join(eb_build.CSRC, f)).read(), f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence'):
        assert word not in code, word


@pytest.fixture(scope='module')
def train_library():
    path = eb_build.build_train()              # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    assert not eb_build.train_needs_build() and open(path + '.srchash').read().strip() == eb_build.train_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in train.TRAIN_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, open(path, 'rb').read()


def test_the_code_object_holds_exactly_the_listed_kernels(train_library):
    lib, blob = train_library
    assert lib.eb_train_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 24.'):]
    for k in KERNELS:
        assert k in section, k
    # the main library exports none of the entries and holds none of the kernels
    main = open(eb_build.build(), 'rb').read()
    for name in list(train.TRAIN_PROTOTYPES) + list(KERNELS):
        assert name.encode() not in main, name


def test_refusals_need_no_device_and_name_their_entry(train_library):
    lib, _ = train_library
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    nan, inf = float('nan'), float('inf')

    def vargs(n=4, stride=1, clip_v=0.2, scale=1.0, **kw):
        full = dict(values=p, ret=p, v_old=p, loss=p, g_values=p)
        full.update(kw)
        return C.byref(train.EbValueLossArgs(n=n, stride=stride, clip_v=clip_v, scale=scale, **full))

    def aargs(n_segments=1, count=4, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, state=p, partials=p, **seg):
        a = train.EbAdamArgs(n_segments=n_segments, lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                             max_grad_norm=max_grad_norm, state=state, partials=partials)
        full = dict(params=p, grads=p, m=p, v=p, count=count)
        full.update(seg)
        for k in range(min(n_segments, train.EB_TRAIN_MAX_SEGMENTS)):
            for name, value in full.items():
                setattr(a.segments[k], name, value)
        return C.byref(a)

    calls = [
        ('eb_value_loss', None), ('eb_value_loss', vargs(n=-1)), ('eb_value_loss', vargs(stride=0)), ('eb_value_loss', vargs(values=None)),
        ('eb_value_loss', vargs(ret=None)), ('eb_value_loss', vargs(scale=nan)), ('eb_value_loss', vargs(clip_v=nan)),
        ('eb_value_loss', vargs(clip_v=-0.1)),
        ('eb_adam_step', None), ('eb_adam_step', aargs(n_segments=33)), ('eb_adam_step', aargs(n_segments=-1)),
        ('eb_adam_step', aargs(count=-1)), ('eb_adam_step', aargs(count=2 ** 31)), ('eb_adam_step', aargs(params=None)),
        ('eb_adam_step', aargs(grads=None)), ('eb_adam_step', aargs(m=None)), ('eb_adam_step', aargs(v=None)),
        ('eb_adam_step', aargs(params=p + 2)), ('eb_adam_step', aargs(grads=p + 1)), ('eb_adam_step', aargs(state=None)),
        ('eb_adam_step', aargs(partials=None)), ('eb_adam_step', aargs(state=p + 4)), ('eb_adam_step', aargs(partials=p + 4)),
        ('eb_adam_step', aargs(lr=nan)), ('eb_adam_step', aargs(lr=-1.0)), ('eb_adam_step', aargs(beta1=nan)), ('eb_adam_step', aargs(beta1=1.0)),
        ('eb_adam_step', aargs(beta2=nan)), ('eb_adam_step', aargs(beta2=-0.1)), ('eb_adam_step', aargs(eps=nan)),
        ('eb_adam_step', aargs(weight_decay=nan)), ('eb_adam_step', aargs(weight_decay=-0.01)), ('eb_adam_step', aargs(max_grad_norm=nan)),
    ]
    assert C.addressof(buf) % 8 == 0
    for name, a in calls:
        assert getattr(lib, name)(a) == -1, name
        assert lib.eb_train_last_error().startswith(name.encode() + b':'), (name, lib.eb_train_last_error())
    assert all(v == 0.0 for v in buf)
    # n = 0 and a total count of 0 are no-ops that need no pointer and no device; a clip_v is not read without v_old
    assert lib.eb_value_loss(C.byref(train.EbValueLossArgs(n=0, stride=1, scale=1.0))) == 0
    assert lib.eb_adam_step(C.byref(train.EbAdamArgs(n_segments=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8))) == 0
    assert lib.eb_adam_step(aargs(n_segments=32, count=0, params=None, grads=None, m=None, v=None, state=None, partials=None)) == 0
    assert all(v == 0.0 for v in buf)


# ---- 3: adam_reference against torch's optimisers ------------------------------------------------------------------------------------------
LR = 3e-3
ADAM_RUNS = [(1000, 200, 0.0), (100000, 20, 0.01), (5000, 50, 0.0)]               # (elements, steps, weight_decay)


def adam_inputs(n, steps, seed=0):
    """parameters N(0, 1) and `steps` gradients spread over four decades"""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n)
    spread = 10.0 ** rng.uniform(-3.0, 1.0, n)
    return p0, [rng.standard_normal(n) * spread for _ in range(steps)]


def torch_run(p0, grads, wd, max_norm, dtype):
    import torch
    p = torch.tensor(p0, dtype=dtype, requires_grad=True)
    opt = (torch.optim.AdamW if wd else torch.optim.Adam)([p], lr=LR, weight_decay=wd)
    norms = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm)))
        opt.step()
    return p.detach().numpy().astype(np.float64), norms


def reference_run(p0, grads, wd, max_norm, dtype, pieces=1):
    cut = lambda a: np.array_split(np.asarray(a, dtype), pieces)
    p, m, v, st = cut(p0), cut(np.zeros_like(p0)), cut(np.zeros_like(p0)), None
    coefs = []
    for g in grads:
        p, m, v, st = train.adam_reference(p, cut(g), m, v, st, lr=LR, weight_decay=wd, max_grad_norm=max_norm, dtype=dtype)
        coefs.append(float(st['coef']))
    assert st['step'] == len(grads) and abs(st['b1t'] - 0.9 ** len(grads)) <= 1e-12 * 0.9 ** len(grads)
    return np.concatenate(p).astype(np.float64), coefs


@pytest.fixture(scope='module')
def adam_yardsticks():
    """per (run, max_norm): the inputs, torch's float64 result and torch's float32 result — computed once, shared by the tests below"""
    import torch
    out = {}
    for n, steps, wd in ADAM_RUNS:
        p0, grads = adam_inputs(n, steps)
        for max_norm in (None, 1.0, 1e6):
            if max_norm is not None and n != 5000:
                continue
            out[(n, steps, wd, max_norm)] = (p0, grads, torch_run(p0, grads, wd, max_norm, torch.float64)[0],
                                             torch_run(p0, grads, wd, max_norm, torch.float32)[0])
    return out


def test_adam_reference_float64_equals_torch_float64(adam_yardsticks):
    for (n, steps, wd, max_norm), (p0, grads, want, _) in adam_yardsticks.items():
        got, coefs = reference_run(p0, grads, wd, max_norm, np.float64, pieces=3)
        within(got, want, 1e-12, 'Adam float64, %d elements, %d steps, wd %g, max norm %r' % (n, steps, wd, max_norm))
        if max_norm == 1.0:
            assert all(c < 1.0 for c in coefs)                       # this norm clips at every step
        if max_norm == 1e6:
            assert all(c == 1.0 for c in coefs)                      # and this one never does
            assert np.array_equal(got, reference_run(p0, grads, wd, None, np.float64)[0])


def test_adam_reference_float32_is_within_4e_of_float64(adam_yardsticks):
    """the project's 4 E rule: E is torch's own float32 Adam's distance from the float64 run on the same inputs"""
    for (n, steps, wd, max_norm), (p0, grads, want, torch32) in adam_yardsticks.items():
        got, _ = reference_run(p0, grads, wd, max_norm, np.float32)
        E = np.abs(torch32 - want).max()
        err = np.abs(got - want).max()
        print('Adam float32, %d elements, %d steps, wd %g, max norm %r: error %.3g, E %.3g, ratio %.2f' % (n, steps, wd, max_norm, err, E, err / E))
        assert err <= 4.0 * E + 2.0 ** -20 * np.abs(want).max()


def test_adam_reference_segments_do_not_matter_and_inputs_are_left_alone():
    p0, grads = adam_inputs(1000, 3)
    one, _ = reference_run(p0, grads, 0.01, 1.0, np.float32)
    many, _ = reference_run(p0, grads, 0.01, 1.0, np.float32, pieces=7)
    assert np.array_equal(one, many)
    p = [p0.astype(np.float32)]
    keep = p[0].copy()
    train.adam_reference(p, [grads[0]], [np.zeros(1000)], [np.zeros(1000)], dtype=np.float32)
    assert np.array_equal(p[0], keep)


# ---- 4: value_loss_reference against torch float64 autograd ----------------------------------------------------------------------------------
def value_case(n=4000, c=0.25, seed=3):
    """Two kinds of rows.  The first half: v_old N(0, 1), v = v_old + dv with dv uniform in [-2.5c, 2.5c] and rows at dv = +-c, 0 and
    +-c / 2 — c a power of two and v_old a short binary fraction there, so that v - v_old is EXACTLY that; returns on both sides of both
    candidates, so that the clipped square is the larger one on about half of the rows outside the interval.  Here v - v_old is exact
    or rounds back, so inside the interval the two squares tie.
    The second half is the real case: v (0.05 N(0, 1) over two decades) drawn INDEPENDENTLY of v_old (uniform in +-0.3) — the network's
    output against a stored value —,
    so that v - v_old is a rounded difference wherever the magnitudes are more than a factor of two apart, v_old + (v - v_old) misses v
    by a unit in the last place, and the squares differ inside the interval too; the returns sit within 1e-6 .. 1 of v, on both sides.
    (A row whose v - v_old rounds to just beyond +-c while v_old +- c rounds to v is the tie outside the interval that the header splits
    otherwise than torch: the tests stay off it.)"""
    rng = np.random.default_rng(seed)
    k = n // 2
    v_old = rng.standard_normal(n)
    dv = rng.uniform(-2.5 * c, 2.5 * c, n)
    v_old[:5] = [0.5, -0.75, 1.25, 0.375, -1.5]
    dv[:5] = [c, -c, 0.0, c / 2, -c / 2]
    v = v_old + dv
    ret = v_old + rng.uniform(-3.0 * c, 3.0 * c, n)
    v_old[k:] = rng.uniform(-0.3, 0.3, n - k)                        # mostly inside the interval, a few rows outside
    v[k:] = 0.05 * rng.standard_normal(n - k) * 10.0 ** rng.uniform(-2.0, 0.0, n - k)
    ret[k:] = v[k:] + rng.standard_normal(n - k) * 10.0 ** rng.uniform(-6.0, 0.0, n - k)
    return v, ret, v_old


def torch_value_loss(v, ret, v_old, c, scale):
    import torch
    x = torch.tensor(np.asarray(v, np.float64), requires_grad=True)
    r = torch.tensor(np.asarray(ret, np.float64))
    if v_old is None:
        loss = 0.5 * (x - r) ** 2
    else:
        o = torch.tensor(np.asarray(v_old, np.float64))
        loss = 0.5 * torch.max((x - r) ** 2, (o + (x - o).clamp(-c, c) - r) ** 2)
    (scale * loss.sum()).backward()
    return loss.detach().numpy(), x.grad.numpy()


def test_value_loss_reference_float64_equals_torch_autograd():
    c, scale = 0.25, 0.5 / 4000
    v, ret, v_old = value_case()
    loss, g = train.value_loss_reference(v, ret, v_old, c, scale, dtype=np.float64)
    want_loss, want_g = torch_value_loss(v, ret, v_old, c, scale)
    within(loss, want_loss, 1e-12, 'clipped value loss')
    within(g, want_g, 1e-12, 'its gradient')
    half = len(v) // 2
    assert np.array_equal(loss[:half], want_loss[:half]) and np.array_equal(g[:half], want_g[:half])     # the same operations: exactly 0
    print('largest differences from torch: loss %.3g, gradient %.3g' % (np.abs(loss - want_loss).max(), np.abs(g - want_g).max()))
    dv = v - v_old
    inside = (dv >= -c) & (dv <= c)
    e1, e2 = v - ret, (v_old + np.clip(dv, -c, c)) - ret
    second = e2 * e2 > e1 * e1
    # all four regions: inside / outside the interval x the clipped square the larger / not the larger one.  Inside, the squares tie
    # where v - v_old is exact (the first half) and differ where it is a rounded difference (the second half): with the clipped one the
    # larger the row returns scale * e2 through the passing clamp, as autograd does — the arm `inside ? e2` that only these rows reach
    count = {(i, s): int(((inside == i) & (second == s)).sum()) for i in (False, True) for s in (False, True)}
    print('rows per (inside, clipped larger):', count)
    assert count[(False, False)] > 300 and count[(False, True)] > 300 and count[(True, False)] > 300 and count[(True, True)] > 30
    assert (e2[:half][inside[:half]] == e1[:half][inside[:half]]).all()      # the constructed rows tie inside
    differ = inside & (e2 != e1)
    assert differ[half:].sum() > 100                                         # the independent rows: vc != v on many of them
    took_e2 = inside & second
    assert np.array_equal(g[took_e2], scale * e2[took_e2]) and (e2[took_e2] != e1[took_e2]).all() and (want_g[took_e2] != 0.0).all()
    assert (~inside).sum() > 1500 and inside[:5].all()                       # dv = +-c, 0, +-c / 2 are inside
    assert (g[second & ~inside] == 0.0).all() and (g[~(second & ~inside)] != 0.0).all()
    # float32 against float64 on float32-representable inputs: tests/test_policy_logp_host.py's bar, 1e-5 of each tensor's maximum
    v, ret, v_old = (a.astype(np.float32) for a in (v, ret, v_old))
    want_loss, want_g = train.value_loss_reference(v, ret, v_old, c, scale, dtype=np.float64)
    loss32, g32 = train.value_loss_reference(v, ret, v_old, c, scale, dtype=np.float32)
    assert loss32.dtype == g32.dtype == np.float32
    # a row whose two squares are within rounding of each other may take the other branch in float32; where the clamp then blocks, the
    # gradient is 0 instead of scale * e: such rows are compared on the loss only
    same_branch = (g32 == 0.0) == (want_g == 0.0)
    print('rows that change branch in float32: %d' % int((~same_branch).sum()))
    assert (~same_branch).sum() <= 4
    within(loss32, want_loss, 1e-5, 'float32 loss against float64')
    within(g32[same_branch], want_g[same_branch], 1e-5, 'float32 gradient against float64')


@pytest.mark.parametrize('c', [0.0, 0.25])
def test_value_loss_reference_without_v_old_and_with_clip_zero(c):
    v, ret, v_old = value_case(n=500, c=max(c, 0.25))
    scale = 1.0 / 500
    loss, g = train.value_loss_reference(v, ret, None, c, scale, dtype=np.float64)
    want_loss, want_g = torch_value_loss(v, ret, None, c, scale)
    within(loss, want_loss, 1e-12, 'unclipped value loss')
    within(g, want_g, 1e-12, 'its gradient')
    assert np.array_equal(g, scale * (v - ret))
    loss, g = train.value_loss_reference(v, ret, v_old, c, None, dtype=np.float64)
    want_loss, want_g = torch_value_loss(v, ret, v_old, c, scale)
    within(loss, want_loss, 1e-12, 'value loss, clip_v %g' % c)
    within(g, want_g, 1e-12, 'its gradient, clip_v %g' % c)


def test_a_nan_poisons_its_own_row_only():
    v, ret, v_old = (a.astype(np.float32) for a in value_case(n=64))
    for k, a in enumerate((v, ret, v_old)):
        a[10 + k] = np.nan
    loss, g = train.value_loss_reference(v, ret, v_old, 0.2, 1.0)
    bad = np.zeros(64, bool)
    bad[10:12] = True                                                # a NaN in v or ret: the row is NaN, and no other row is
    assert np.isnan(loss[bad]).all() and np.isnan(g[bad]).all() and np.isfinite(loss[~bad]).all() and np.isfinite(g[~bad]).all()
    plain = train.value_loss_reference(v, ret, None, 0.0, 1.0)       # a NaN in v_old alone: every comparison fails, the unclipped row
    assert loss[12] == plain[0][12] and g[12] == plain[1][12]
