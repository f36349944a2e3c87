"""CPU (-m "not gpu"): the update-control family (include/envbuild_ctl.h, env_build_amd.ctl) — its header against the module's binding
table and argument structs, the separation of libenvbuild_ctl.so from the other four libraries and the kernels its code object holds,
device-free refusals, and the three NumPy restatements: the table's clamp, the KL against fold_log(ppo_log_reference) bit for bit with
the sticky stop, and the controlled Adam against adam_reference at the scaled learning rate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import ctl, epoch, train
from tests import _ctl as T
from tests import _kernel_census as K
from tests._helpers import ROOT

STRUCTS = {'eb_ctl_begin_args': ctl.EbCtlBeginArgs, 'eb_kl_stop_args': ctl.EbKlStopArgs, 'eb_adam_ctl_args': ctl.EbAdamCtlArgs}


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(ctl.CTL_PROTOTYPES) == sorted(T.ENTRIES + ('eb_ctl_abi_version', 'eb_ctl_last_error'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in STRUCTS.items()}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, args) in ctl.CTL_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert len(params) <= 1 and not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    assert not [n for n in names + list(T.KERNELS) if re.search(r'_gate(d|_|$)', n)]
    macros = {m: getattr(ctl, m) for m in ('EB_CTL_ABI_VERSION', 'EB_CTL_KL_BLOCKS')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_CTL_\w+) ', text)) == sorted(macros)
    assert tuple(macros.values()) == (1, 64) and ctl.EB_CTL_KL_BLOCKS == epoch.EB_EPOCH_LOG_BLOCKS
    assert T.struct_fields(src, 'eb_update_ctl') == list(ctl.EbUpdateCtl._fields_)
    assert [k for k, _ in ctl.EbUpdateCtl._fields_] == list(ctl.FIELDS)
    assert C.sizeof(ctl.EbUpdateCtl) == 32 and C.alignment(ctl.EbUpdateCtl) == 8
    assert ctl.EbUpdateCtl.last_kl.offset == 24 and ctl.EbUpdateCtl.lr_scale.offset == 8
    for name, struct in STRUCTS.items():
        assert T.struct_fields(src, name, {'eb_adam_args': train.EbAdamArgs}) == list(struct._fields_), name
    for struct in (ctl.EbCtlBeginArgs, ctl.EbKlStopArgs, train.EbAdamArgs):                   # eb_adam_step_ctl's stream is adam.stream
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    assert ctl.EbAdamCtlArgs.adam.offset == 0 and ctl.EbAdamCtlArgs.ctl.offset == C.sizeof(train.EbAdamArgs)
    for words in ('bit for bit', 'AT CALL TIME', 'tests/test_stream_census.py', 'ALWAYS exactly TWO launches', 'ONE launch',
                  'libenvbuild_ctl.so ONLY', 'eb_ctl_last_error', 'begin_reference', 'kl_stop_reference', 'adam_ctl_reference',
                  'zero-filled block is a valid state BEFORE the first', 'a NaN KL stops', 'cannot branch', 'not time',
                  'returns before its first store', 'no last-block ticket', 'the bits are the caller\'s'):
        assert words in text, words


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import collect, ppo
    others = (set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES) | set(epoch.EPOCH_PROTOTYPES)
              | set(collect.COLLECT_PROTOTYPES))
    assert not set(ctl.CTL_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(ctl.CTL_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in ctl.__all__]
    # the subclasses are subclasses: what takes the parents takes them
    assert issubclass(ctl.Adam, train.Adam) and issubclass(ctl.PPOUpdate, train.PPOUpdate) and issubclass(ctl.PPOEpochs, epoch.PPOEpochs)
    assert ctl.PPOEpochs.capture is epoch.PPOEpochs.capture and ctl.PPOEpochs.replay is epoch.PPOEpochs.replay
    assert ctl.PPOUpdate.step is train.PPOUpdate.step                                           # no restated chain


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_ctl_sources_are_in_no_list_of_the_other_libraries():
    inc = lambda f: os.path.join('..', '..', 'include', f)
    mine = set(T.UNIT) | {inc('envbuild_ctl.h')}
    own = eb_build.CTL_SOURCES + eb_build.CTL_HEADERS
    assert eb_build.CTL_SOURCES == ['eb_ctl.hip'] and mine <= set(own)
    others = [eb_build.SOURCES, eb_build.HEADERS, eb_build.TRAIN_SOURCES, eb_build.TRAIN_HEADERS, eb_build.EPOCH_SOURCES,
              eb_build.EPOCH_HEADERS, eb_build.COLLECT_SOURCES, eb_build.COLLECT_HEADERS] + list(eb_build.KERNEL_SOURCES.values())
    for files in others:
        assert not [f for f in files if 'ctl' in f], files
    # the reverse: of the other libraries only the train family's device header and public header, and the return codes' header
    assert set(own) - mine == {'eb_train_device.h', inc('envbuild_train.h'), inc('envbuild.h')}
    assert set(own) - mine <= set(eb_build.TRAIN_HEADERS)
    assert eb_build.CTL_LIB not in (eb_build.LIB, eb_build.TRAIN_LIB, eb_build.EPOCH_LIB, eb_build.COLLECT_LIB)
    assert os.path.dirname(eb_build.CTL_LIB) == os.path.dirname(eb_build.LIB) and os.path.basename(eb_build.CTL_LIB) == 'libenvbuild_ctl.so'
    assert len({eb_build.ctl_source_hash(), eb_build.collect_source_hash(), eb_build.epoch_source_hash(), eb_build.train_source_hash(),
                eb_build.source_hash()}) == 5
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_ctl.hip']
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen:
            continue
        seen.add(f)
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            for included in re.findall(r'#include "([^"]+)"', fh.read()):
                todo.append(os.path.join(os.path.dirname(f), included))
    listed = {os.path.normpath(f) for f in own}
    assert seen == listed, (sorted(seen - listed), sorted(listed - seen))
    # no unit of the other libraries includes a ctl header
    for f in set(sum(others[:8], [])):
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            body = fh.read()
        assert 'eb_ctl' not in body and 'envbuild_ctl' not in body, f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly, nothing allocates, copies or synchronises
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence', 'hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in code, word
    assert 'train::fold' in code and 'train::adam_element' in code and 'long long' in code
    assert code.count('hipLaunchKernelGGL') == 5 and set(re.findall(r'__global__[^\n]*void (\w+)\(', code)) == set(T.KERNELS)


def test_the_code_object_holds_exactly_the_five_kernels():
    lib, blob = T.library()
    assert lib.eb_ctl_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 27.'):]
    for k in T.KERNELS:
        assert k in section, k
    # the other four libraries export none of the entries and hold none of the kernels
    for path in (eb_build.build(), eb_build.build_train(), eb_build.build_epoch(), eb_build.build_collect()):
        other = open(path, 'rb').read()
        for name in list(ctl.CTL_PROTOTYPES) + list(T.KERNELS):
            assert name.encode() not in other, (path, name)


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    nan = float('nan')

    def bargs(**kw):
        full = dict(ctl=p, lr_table=p, n_table=3)
        full.update(kw)
        return C.byref(ctl.EbCtlBeginArgs(**full))

    def kargs(**kw):
        full = dict(n=4, logp=p, logp_old=p, limit=0.02, ctl=p, partials=p, log=p, max_slots=4)
        full.update(kw)
        return C.byref(ctl.EbKlStopArgs(**full))

    def aargs(n_segments=1, count=4, ctl_=p, **kw):
        a = ctl.EbAdamCtlArgs(ctl=ctl_)
        scalars = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, state=p, partials=p)
        seg = dict(params=p, grads=p, m=p, v=p, count=count)
        for k, v in kw.items():
            (scalars if k in scalars else seg)[k] = v
        a.adam.n_segments = n_segments
        for k, v in scalars.items():
            setattr(a.adam, k, v)
        for s in range(min(max(n_segments, 0), train.EB_TRAIN_MAX_SEGMENTS)):
            for k, v in seg.items():
                setattr(a.adam.segments[s], k, v)
        return C.byref(a)

    calls = [('eb_ctl_begin', None), ('eb_ctl_begin', bargs(ctl=None)), ('eb_ctl_begin', bargs(ctl=p + 4)), ('eb_ctl_begin', bargs(lr_table=p + 2)),
             ('eb_ctl_begin', bargs(n_table=0)), ('eb_ctl_begin', bargs(n_table=-1))]
    calls += [('eb_kl_stop', None), ('eb_kl_stop', kargs(n=-1)), ('eb_kl_stop', kargs(n=2 ** 31)), ('eb_kl_stop', kargs(limit=nan)),
              ('eb_kl_stop', kargs(max_slots=-1)), ('eb_kl_stop', kargs(ctl=None)), ('eb_kl_stop', kargs(ctl=p + 4)),
              ('eb_kl_stop', kargs(log=p + 4)), ('eb_kl_stop', kargs(partials=None)), ('eb_kl_stop', kargs(partials=p + 4)),
              ('eb_kl_stop', kargs(n=0, ctl=None)), ('eb_kl_stop', kargs(n=0, limit=nan))]
    calls += [('eb_kl_stop', kargs(**{k: v})) for k in ('logp', 'logp_old') for v in (None, p + 2)]
    calls += [('eb_adam_step_ctl', None), ('eb_adam_step_ctl', aargs(ctl_=None)), ('eb_adam_step_ctl', aargs(ctl_=p + 4)),
              ('eb_adam_step_ctl', aargs(ctl_=None, n_segments=0)),
              ('eb_adam_step_ctl', aargs(n_segments=33)), ('eb_adam_step_ctl', aargs(n_segments=-1)), ('eb_adam_step_ctl', aargs(count=-1)),
              ('eb_adam_step_ctl', aargs(count=2 ** 31)), ('eb_adam_step_ctl', aargs(params=None)), ('eb_adam_step_ctl', aargs(grads=None)),
              ('eb_adam_step_ctl', aargs(m=None)), ('eb_adam_step_ctl', aargs(v=None)), ('eb_adam_step_ctl', aargs(params=p + 2)),
              ('eb_adam_step_ctl', aargs(grads=p + 1)), ('eb_adam_step_ctl', aargs(state=None)), ('eb_adam_step_ctl', aargs(partials=None)),
              ('eb_adam_step_ctl', aargs(state=p + 4)), ('eb_adam_step_ctl', aargs(partials=p + 4)), ('eb_adam_step_ctl', aargs(lr=nan)),
              ('eb_adam_step_ctl', aargs(lr=-1.0)), ('eb_adam_step_ctl', aargs(beta1=nan)), ('eb_adam_step_ctl', aargs(beta1=1.0)),
              ('eb_adam_step_ctl', aargs(beta2=nan)), ('eb_adam_step_ctl', aargs(beta2=-0.1)), ('eb_adam_step_ctl', aargs(eps=nan)),
              ('eb_adam_step_ctl', aargs(weight_decay=nan)), ('eb_adam_step_ctl', aargs(weight_decay=-0.01)),
              ('eb_adam_step_ctl', aargs(max_grad_norm=nan))]
    assert len(calls) >= 50 and {name for name, _ in calls} == set(T.ENTRIES)
    for k, (name, a) in enumerate(calls):
        assert getattr(lib, name)(a) == -1, (name, k)
        assert lib.eb_ctl_last_error().startswith(name.encode() + b':'), (name, lib.eb_ctl_last_error())
    assert all(v == 0.0 for v in buf)
    # no rows and no elements: no-ops that need no pointer but ctl's and no device
    assert lib.eb_kl_stop(kargs(n=0, logp=None, logp_old=None, partials=None, log=None, max_slots=0)) == 0
    assert lib.eb_adam_step_ctl(aargs(n_segments=0, state=None, partials=None)) == 0
    assert lib.eb_adam_step_ctl(aargs(n_segments=32, count=0, params=None, grads=None, m=None, v=None, state=None, partials=None)) == 0
    assert all(v == 0.0 for v in buf)


# ---- 4: begin_reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', [None, [0.75], [1.0, 0.5, 0.0]])
def test_begin_reference_walks_the_table_and_holds_its_last_entry(table):
    c = None
    for it in range(5):
        if c is not None:                                          # whatever the iteration left behind is cleared
            c.update(stopped=1, slot=7, stopped_at=3, last_kl=0.25)
        c = ctl.begin_reference(c, table)
        want = np.float32(1.0) if table is None else np.float32(table[min(it, len(table) - 1)])
        assert T.same_ctl(c, dict(iteration=it + 1, lr_scale=want, stopped=0, slot=0, stopped_at=-1, last_kl=0.0)), (table, it, c)
        assert type(c['lr_scale']) is np.float32
    with pytest.raises(ValueError):
        ctl.begin_reference(None, [])


# ---- 5: kl_stop_reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', T.KL_SIZES)
def test_kl_stop_reference_is_fold_logs_approx_kl_bit_for_bit(n):
    logp, logp_old = T.kl_rows(n)
    want = T.kl_of(logp, logp_old)
    assert np.isfinite(want) and want != 0.0
    above, below = np.nextafter(want, np.inf), np.nextafter(want, -np.inf)
    log = np.full((3, 2), T.SENTINEL)
    c0 = ctl.begin_reference(None, None)
    c1, kl = ctl.kl_stop_reference(c0, logp, logp_old, want, log)            # kl <= limit holds with equality: no stop
    assert kl == want and T.same_ctl(c1, T.live(slot=1, last_kl=want)) and c0['slot'] == 0
    c2, kl = ctl.kl_stop_reference(c1, logp, logp_old, above, log)
    assert kl == want and T.same_ctl(c2, T.live(slot=2, last_kl=want))
    c3, kl = ctl.kl_stop_reference(c2, logp, logp_old, below, log)           # the limit one unit below the value: stop, at slot 2
    assert T.same_ctl(c3, T.live(stopped=1, slot=3, stopped_at=2, last_kl=want))
    assert np.array_equal(log, [[want, 1.0], [want, 1.0], [want, 0.0]])
    c4, kl = ctl.kl_stop_reference(c3, logp, logp_old, above, log)           # sticky; and the log's fourth slot does not exist
    assert T.same_ctl(c4, T.live(stopped=1, slot=4, stopped_at=2, last_kl=want)) and log.shape == (3, 2)
    # the order matters at these sizes: the plain float64 mean is close, and the restatement is not obliged to equal it
    plain = float(np.mean((logp_old - logp).astype(np.float64)))
    assert abs(plain - want) <= 1e-12 * float(np.abs(logp_old - logp).sum()) / n


def test_kl_stop_reference_nan_sticky_and_cleared_by_begin():
    n = 300
    logp, logp_old = T.kl_rows(n)
    small = T.kl_of(logp, logp_old)
    bad = logp.copy()
    bad[123] = np.nan
    assert np.isnan(T.kl_of(bad, logp_old))
    log = np.full((8, 2), T.SENTINEL)
    c = ctl.begin_reference(None, [0.5])
    c, kl = ctl.kl_stop_reference(c, logp, logp_old, 1.0, log)
    assert c['stopped'] == 0 and kl == small
    c, kl = ctl.kl_stop_reference(c, bad, logp_old, 1.0, log)                # a planted NaN stops, under any limit
    assert np.isnan(kl) and T.same_ctl(c, T.live(0.5, stopped=1, slot=2, stopped_at=1, last_kl=np.nan))
    for s in (2, 3):                                                         # later slots with a small KL: still stopped, at slot 1
        c, kl = ctl.kl_stop_reference(c, logp, logp_old, 1.0, log)
        assert kl == small and T.same_ctl(c, T.live(0.5, stopped=1, slot=s + 1, stopped_at=1, last_kl=small))
    assert np.array_equal(log[:4, 1], [1.0, 0.0, 0.0, 0.0]) and np.isnan(log[1, 0]) and (log[4:] == T.SENTINEL).all()
    assert np.array_equal(log[[0, 2, 3], 0], [small] * 3)
    inf_limit, _ = ctl.kl_stop_reference(ctl.begin_reference(None), bad, logp_old, np.inf)
    assert inf_limit['stopped'] == 1                                         # !(NaN <= inf)
    c = ctl.begin_reference(c, [0.5])
    assert T.same_ctl(c, dict(T.live(0.5), iteration=2))
    c, _ = ctl.kl_stop_reference(c, logp, logp_old, 1.0)
    assert c['stopped'] == 0 and c['slot'] == 1
    # no rows: the block is left alone; a NaN limit is refused
    same, kl = ctl.kl_stop_reference(c, logp[:0], logp_old[:0], 1.0, log)
    assert kl is None and T.same_ctl(same, c)
    with pytest.raises(ValueError):
        ctl.kl_stop_reference(c, logp, logp_old, np.nan)


# ---- 6: adam_ctl_reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 0.5, 0.0, 0.3])
def test_adam_ctl_reference_is_adam_reference_at_the_scaled_learning_rate(scale):
    rng = np.random.default_rng(6)
    counts = [5, 0, 1030]
    p = [rng.standard_normal(c).astype(np.float32) for c in counts]
    g = [rng.standard_normal(c).astype(np.float32) for c in counts]
    m, v = [np.zeros(c, np.float32) for c in counts], [np.zeros(c, np.float32) for c in counts]
    kw = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=0.5)
    lr = 3e-3
    got, want = (p, m, v, None), (p, m, v, None)
    for _ in range(2):
        got = ctl.adam_ctl_reference(T.live(scale), got[0], g, got[1], got[2], got[3], lr=lr, **kw)
        want = train.adam_reference(want[0], g, want[1], want[2], want[3], lr=lr * float(np.float32(scale)), **kw)
        for a, b in zip(got[:3], want[:3]):
            assert all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b))
        assert got[3] == want[3]
    if scale == 1.0:
        plain = train.adam_reference(p, g, m, v, None, lr=lr, **kw)
        first = ctl.adam_ctl_reference(T.live(1.0), p, g, m, v, None, lr=lr, **kw)
        assert all(np.array_equal(x, y) for a, b in zip(first[:3], plain[:3]) for x, y in zip(a, b)) and first[3] == plain[3]
    if scale == 0.0:                                              # the moments and the step count move, the parameters only by the decay's 0
        assert all(np.array_equal(x, y) for x, y in zip(got[0], p)) and got[3]['step'] == 2 and np.abs(got[1][2]).max() > 0
    # stopped: the inputs, as they are
    held = ctl.adam_ctl_reference(T.live(scale, stopped=1, stopped_at=0, slot=1), got[0], g, got[1], got[2], got[3], lr=lr, **kw)
    for a, b in zip(held[:3], got[:3]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert held[3] == got[3]
    fresh = ctl.adam_ctl_reference(T.live(scale, stopped=1), p, g, m, v, None, lr=lr, **kw)
    assert fresh[3] == dict(step=0, b1t=0.0, b2t=0.0) and all(np.array_equal(x, y) for x, y in zip(fresh[0], p))
