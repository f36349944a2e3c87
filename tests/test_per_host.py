"""CPU (-m "not gpu"): the prioritised-replay family (include/envbuild_per.h, env_build_amd.per) — its header against the module's binding
table and argument structs, the separation of libenvbuild_per.so from the other eight libraries and the kernels its code object holds,
device-free refusals and no-ops, and the NumPy restatements: the tree's layout against the header's formula and its sums against plain
loops, the descent's guarantees (a drawn leaf is positive, a lone last leaf is always drawn, every prefix boundary, the fallback), the
write-back's last-writer rule, coarse proportionality, and the weight and the new priority against float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import offpolicy as O
from env_build_amd import per as P
from tests import _kernel_census as K
from tests import _per as T
from tests._helpers import ROOT

OTHERS = ('', 'train_', 'epoch_', 'collect_', 'ctl_', 'ac_', 'norm_', 'offpolicy_')


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(P.PER_PROTOTYPES) == sorted(T.ENTRIES + ('eb_per_abi_version', 'eb_per_last_error', 'eb_per_tree_doubles',
                                                                    'eb_per_set_launches'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in T.STRUCTS.items()}
    kinds['int32_t'] = C.c_int32
    results = {'int': C.c_int, 'const char*': C.c_char_p, 'int64_t': C.c_int64}
    for name, (res, args) in P.PER_PROTOTYPES.items():
        m = re.search(r'(\bint|\bint64_t|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        if name in T.ENTRIES:
            assert [kinds[p] for p in params] == args, name                   # no parameter name: the type is the whole parameter
        else:
            assert [kinds[p.split()[0]] for p in params] == args, name        # the two geometry queries take scalars by name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    macros = {m: getattr(P, m) for m in ('EB_PER_ABI_VERSION', 'EB_PER_RADIX', 'EB_PER_MAX_LEVELS', 'EB_PER_SMALL_NODES', 'EB_PER_MIN_BLOCKS',
                                         'EB_PER_ROUTE_RANGE', 'EB_PER_ROUTE_INDEXED')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert tuple(macros.values()) == (1, 32, 7, 1024, 64, 0, 1)
    for macro, value in (('EB_PER_PRIO_MIN', 2.0 ** -40), ('EB_PER_PRIO_MAX', 2.0 ** 40)):
        lit = re.search(r'#define %s ([0-9.e+-]+)f' % macro, text).group(1)
        assert np.float32(lit) == np.float32(value) == np.float32(getattr(P, macro)), macro
    assert sorted(re.findall(r'#define (EB_PER_\w+) ', text)) == sorted(list(macros) + ['EB_PER_PRIO_MIN', 'EB_PER_PRIO_MAX'])
    for name, struct in T.STRUCTS.items():
        assert T.fields_of(src, name) == list(struct._fields_), name
        assert struct._fields_[-1] == ('stream', C.c_void_p)                 # each argument struct carries `void* stream`
    for words in ('libenvbuild_per.so ONLY', 'eb_per_last_error', 'AT CALL TIME', 'tests/test_stream_census.py', 'ONE launch', 'INVARIANT',
                  'THE HIGHEST ROW NUMBER WINS', 'big(C) + 2', 'big(C) + 3', 'LAST child with s_c > 0', 'sequential ascending', '0x7FC00000',
                  'min_partials', 'No float atomics, no last-block ticket', 'tree_reference', 'set_reference', 'sample_reference',
                  'weigh_reference', 'the root is the last double', 'exactly 1 on the row of the minimum', 'indices = eb_per_sample'):
        assert words in text, words


def test_the_capture_test_holds_every_entry_as_the_struct_census_asks():
    """tests/_capture_cases.py's tables are fixed lists of the other families' entries; the header declares these four prototypes without a
    parameter name, which that parser passes over.  The obligation itself is applied here, with the census's own function_text: the named
    GPU test mentions the entry, runs it on a side stream, captures and replays it."""
    from tests._capture_cases import STRUCT_STREAM_HELD, function_text, stream_entries, struct_stream_entries
    _, src = T.header()
    text = function_text('test_gpu_per', 'test_every_entry_on_a_side_stream_and_under_capture')
    assert text is not None and 'side' in text and re.search(r'\bcapture\(', text) and 'replay' in text
    for entry in T.ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*\)\s*;' % (entry, T.STRUCT_OF[entry]), src), entry
        assert ('stream', C.c_void_p) in T.fields_of(src, T.STRUCT_OF[entry])
        assert entry not in STRUCT_STREAM_HELD and entry not in struct_stream_entries() and entry not in stream_entries()
        assert re.search(r"['\"]%s['\"]" % entry, text), entry
    assert len(struct_stream_entries()) == 20 and len(stream_entries()) == 50


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import ac, collect, ctl, epoch, norm, ppo, train
    others = (set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES) | set(epoch.EPOCH_PROTOTYPES)
              | set(collect.COLLECT_PROTOTYPES) | set(ctl.CTL_PROTOTYPES) | set(ac.AC_PROTOTYPES) | set(norm.NORM_PROTOTYPES)
              | set(O.OFFPOLICY_PROTOTYPES))
    assert not set(P.PER_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(P.PER_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in P.__all__]
    assert O.SAC.KERNELS == 42 and issubclass(P.SAC, O.SAC) and issubclass(P.PrioritizedReplayBuffer, O.ReplayBuffer)
    assert 'step' not in P.SAC.__dict__ and 'capture' not in P.SAC.__dict__ and 'replay' not in P.SAC.__dict__      # it restates no chain


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_per_sources_are_in_no_list_of_the_other_libraries():
    header = os.path.join('..', '..', 'include', 'envbuild_per.h')
    mine = set(T.UNIT) | {header}
    own = eb_build.PER_SOURCES + eb_build.PER_HEADERS
    assert eb_build.PER_SOURCES == ['eb_per.hip'] and mine <= set(own)
    lists = [getattr(eb_build, (p.upper() + kind)) for p in OTHERS for kind in ('SOURCES', 'HEADERS')]
    for files in lists + list(eb_build.KERNEL_SOURCES.values()):
        assert not [f for f in files if 'eb_per' in f or 'envbuild_per' in f], files
    # what it borrows is read and never changed
    borrowed = set(own) - mine
    assert borrowed == {'eb_offpolicy_device.h', 'eb_policy_sample_device.h', 'eb_mlp_device.h', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h',
                        os.path.join('..', '..', 'include', 'envbuild.h')}
    assert borrowed <= set(eb_build.HEADERS) | set(eb_build.OFFPOLICY_HEADERS)
    libs = [getattr(eb_build, p.upper() + 'LIB') for p in OTHERS]
    assert eb_build.PER_LIB not in libs and os.path.dirname(eb_build.PER_LIB) == os.path.dirname(eb_build.LIB)
    assert os.path.basename(eb_build.PER_LIB) == 'libenvbuild_per.so'
    hashes = {getattr(eb_build, p + 'source_hash')() for p in OTHERS} | {eb_build.per_source_hash()}
    assert len(hashes) == 9
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_per.hip']
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen:
            continue
        seen.add(f)
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            for inc in re.findall(r'#include "([^"]+)"', fh.read()):
                todo.append(os.path.join(os.path.dirname(f), inc))
    listed = {os.path.normpath(f) for f in own}
    assert seen == listed, (sorted(seen - listed), sorted(listed - seen))
    # no unit of the other libraries includes a header of this one
    for files in lists:
        for f in files:
            with open(os.path.join(eb_build.CSRC, f)) as fh:
                body = fh.read()
            assert 'eb_per' not in body and 'envbuild_per' not in body, f
    # kernel code rules: plain C++, __syncthreads only, the two integer atomicMax and no other atomic, no inline assembly, nothing
    # allocates, copies or synchronises
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    assert re.findall(r'\w*[aA]tomic\w*', code) == ['atomicMax', 'atomicMax']
    assert len(re.findall(r'atomicMax\((A\.stamp \+ j|reinterpret_cast<int\*>\(A\.max_prio\)),', code)) == 2          # both on integers
    for word in ('asm', '__builtin_amdgcn', '__shfl', '__threadfence', 'hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in code, word
    assert '__syncthreads' in code and 'long long' in code and code.count('__builtin_fmaf') == 1
    assert '-ffp-contract=off' in eb_build.FLAGS
    # the build entry compiles it; the smoke run is as it was
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    smoke = entry[entry.index('def smoke'):]
    assert '_b.build_per()' in entry and not re.search(r'\bper\b|_per\b|eb_per', smoke)


def test_the_code_object_holds_exactly_the_nine_kernels():
    lib, blob = T.library()
    assert lib.eb_per_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 31.'):]
    for k in T.KERNELS:
        assert k in section, k


# ---- 3: the layout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', T.CAPACITIES + (32768, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1))
def test_offsets_are_the_headers_formula(C_):
    lib, _ = T.library()
    n, off, doubles = T.header_levels(C_)
    have_n, have_off, first_small = P.tree_levels(C_)
    assert have_n == [C_] + n and have_off == [None] + off and P.tree_doubles(C_) == doubles == lib.eb_per_tree_doubles(C_)
    assert len(n) <= P.EB_PER_MAX_LEVELS and doubles <= C_
    small = [k for k in range(1, len(n) + 1) if n[k - 1] <= P.EB_PER_SMALL_NODES]
    assert small == list(range(first_small, len(n) + 1)) and len(small) == min(len(n), 3) and sum(n[k - 1] for k in small) <= 1057
    big = len(n) - len(small)
    assert lib.eb_per_set_launches(C_, P.EB_PER_ROUTE_RANGE) == big + 2 == P.set_launches(C_, P.EB_PER_ROUTE_RANGE)
    assert lib.eb_per_set_launches(C_, P.EB_PER_ROUTE_INDEXED) == big + 3 == P.set_launches(C_, P.EB_PER_ROUTE_INDEXED) <= len(n) + 2
    assert lib.eb_per_tree_doubles(0) == -1 and lib.eb_per_set_launches(C_, 2) == -1 and lib.eb_per_set_launches(0, 0) == -1


@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_tree_reference_is_the_invariant_written_as_loops(C_):
    prio = T.leaves(C_)
    tree = P.tree_reference(prio)
    assert tree.dtype == np.float64 and T.bits(tree, T.tree_by_loops(prio))
    assert tree[-1] > 0 and abs(tree[-1] - prio.astype(np.float64).sum()) <= 1e-12 * tree[-1]
    assert not P.tree_reference(np.zeros(C_, np.float32)).any()


# ---- 4: refusals and no-ops ------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    big, nan = 2 ** 31 - 1, float('nan')
    pointers = {'eb_per_reset': ('prio', 'tree', 'max_prio', 'stamp'),
                'eb_per_set': ('prio', 'tree', 'max_prio', 'stamp', 'index', 'value'),
                'eb_per_sample': ('prio', 'tree', 'counter', 'u_in', 'index_out', 'prio_out', 'noise_id_out', 'min_partials'),
                'eb_per_weigh': ('index', 'prio', 'min_partials', 'q1', 'q2', 'y', 'counter', 'g_q1', 'g_q2', 'loss1', 'loss2', 'w_out', 'prio_new')}
    scalars = {'eb_per_reset': dict(capacity=8), 'eb_per_set': dict(capacity=8, route=1, n=4, start=6),
               'eb_per_sample': dict(capacity=8, m=4, seed=1, draw=2),
               'eb_per_weigh': dict(m=4, beta=0.4, beta_step=0.01, alpha=0.6, eps=1e-6)}

    def args(entry, **kw):
        full = dict(scalars[entry], **{k: p for k in pointers[entry]})
        full.update(kw)
        return C.byref(T.STRUCTS[T.STRUCT_OF[entry]](**full))

    R, St, Sm, W = T.ENTRIES
    calls = [(e, None) for e in T.ENTRIES]
    calls += [(R, args(R, capacity=0)), (R, args(R, capacity=-5)), (R, args(R, tree=p + 4))]
    calls += [(R, args(R, **{k: v})) for k in pointers[R] for v in (None, p + 2)]
    calls += [(St, args(St, capacity=0)), (St, args(St, route=2)), (St, args(St, route=-1)), (St, args(St, n=-1)), (St, args(St, route=0, n=9)),
              (St, args(St, route=0, start=-1)), (St, args(St, route=0, start=8)), (St, args(St, tree=p + 4)), (St, args(St, route=0, tree=None))]
    calls += [(St, args(St, **{k: v})) for k in pointers[St] for v in (None, p + 2)]
    calls += [(St, args(St, route=0, **{k: v})) for k in ('prio', 'max_prio') for v in (None, p + 2)]
    calls += [(Sm, args(Sm, capacity=0)), (Sm, args(Sm, m=-1)), (Sm, args(Sm, tree=p + 4)), (Sm, args(Sm, counter=p + 4)), (Sm, args(Sm, u_in=p + 4))]
    calls += [(Sm, args(Sm, **{k: v})) for k in ('prio', 'tree', 'index_out') for v in (None, p + 2)]
    calls += [(Sm, args(Sm, **{k: p + 2})) for k in ('prio_out', 'noise_id_out', 'min_partials')]
    calls += [(W, args(W, m=-1)), (W, args(W, beta=nan)), (W, args(W, beta_step=nan)), (W, args(W, alpha=nan)), (W, args(W, eps=nan)),
              (W, args(W, g_q1=None, g_q2=None, loss1=None, loss2=None, w_out=None, prio_new=None)), (W, args(W, counter=p + 4)),
              (W, args(W, q1=None)), (W, args(W, y=None))]
    calls += [(W, args(W, **{k: v})) for k in ('index', 'prio', 'min_partials') for v in (None, p + 2)]
    calls += [(W, args(W, **{k: p + 2})) for k in ('q1', 'q2', 'y', 'g_q1', 'g_q2', 'loss1', 'loss2', 'w_out', 'prio_new')]
    assert len(calls) >= 70 and {name for name, _ in calls} == set(T.ENTRIES)
    for k, (name, a) in enumerate(calls):
        assert getattr(lib, name)(a) == -1, (k, name)
        assert lib.eb_per_last_error().startswith(name.encode() + b':'), (name, lib.eb_per_last_error())
    assert all(v == 0.0 for v in buf)
    # no rows: no-ops that need no pointer and no device, on both routes; m = 0 needs no pointer either
    none = lambda e: {k: None for k in pointers[e]}
    assert lib.eb_per_set(args(St, n=0, **none(St))) == 0 and lib.eb_per_set(args(St, route=0, n=0, start=0, **none(St))) == 0
    assert lib.eb_per_sample(args(Sm, m=0, **none(Sm))) == 0 and lib.eb_per_weigh(args(W, m=0, **none(W))) == 0
    assert all(v == 0.0 for v in buf)
    with pytest.raises(ValueError):
        P.tree_levels(0)
    with pytest.raises(ValueError):
        P.set_launches(8, 2)


# ---- 5: the descent ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_a_drawn_leaf_is_positive_and_a_lone_last_leaf_is_always_drawn(C_):
    prio = T.leaves(C_)
    for m, kw in ((1, dict(seed=3)), (257, dict(seed=4, draw=2, base=5)), (4096, dict(seed=5))):
        out = P.sample_reference(prio, m, **kw)
        idx = out['index']
        assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < C_ and (prio[idx] > 0).all()
        assert T.bits(out['prio'], prio[idx]) and (np.diff(idx) >= 0).all()                      # stratified: the draws ascend
        word = O.sample_word_reference(m, kw['seed'], kw.get('draw', 0), kw.get('base', 0))      # eb_replay_sample's keyed word
        assert T.bits(out['noise_id'], (word & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        assert out['min_partials'].min() == prio[idx].min() and out['min_partials'].shape == (64,)
        assert np.isinf(out['min_partials'][min(63, (m - 1) // 256) + 1:]).all()
    lone = np.zeros(C_, np.float32)
    lone[C_ - 1] = 3.5
    out = P.sample_reference(lone, 257, seed=9)
    assert (out['index'] == C_ - 1).all() and (out['prio'] == np.float32(3.5)).all()
    ends = P.sample_reference(lone, 3, u_in=np.array([0.0, 0.5, np.nextafter(1.0, 0.0)]))
    assert (ends['index'] == C_ - 1).all()
    # an empty ring: every index is -1, every priority a quiet NaN, every partial +inf
    out = P.sample_reference(np.zeros(C_, np.float32), 65, seed=1)
    assert (out['index'] == -1).all() and (out['prio'].view(np.uint32) == 0x7FC00000).all() and np.isinf(out['min_partials']).all()


@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_one_double_step_either_side_of_every_prefix_boundary(C_):
    """tests/_per.py: boundary_case — the leaves are small integers, so the hierarchy must give what one flat cumulative sum gives; each
    boundary B_i is approached from the double just below it (leaf i) and hit exactly (the next positive leaf)"""
    prio, u_in, want = T.boundary_case(C_)
    out = P.sample_reference(prio, len(u_in), u_in=u_in)
    assert T.bits(out['index'], want)
    assert set(want.tolist()) == set(np.flatnonzero(prio > 0).tolist())                      # every positive leaf is reached


@pytest.mark.parametrize('C_', T.CAPACITIES)
def test_the_fallback_lands_on_the_last_positive_leaf(C_):
    prio, tree, u_in, last = T.fallback_case(C_)
    out = P.sample_reference(prio, 1, u_in=u_in, tree=tree)
    assert out['index'].tolist() == [last] and prio[last] > 0
    # on the true tree the same draw does not need it: the fallback is what the excess forces
    honest = P.sample_reference(prio, 1, u_in=u_in)
    assert prio[honest['index'][0]] > 0


# ---- 6: the write-back ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C_', [1, 33, 1025])
def test_set_reference_is_last_writer_wins(C_):
    prio0 = T.leaves(C_)
    for m, kind in ((1, 'random'), (64, 'random'), (257, 'random'), (257, 'one'), (2 * C_, 'twice')):
        idx, val = T.write_back_rows(C_, m, kind)
        prio, mx = P.set_reference(prio0, 1.0, index=idx, value=val)
        want, top = prio0.copy(), np.float32(1.0)
        for r in range(len(idx)):                                          # a plain loop in row order
            j, v = int(idx[r]), val[r]
            if 0 <= j < C_ and v > 0 and v < np.inf:
                want[j] = min(max(v, np.float32(2.0 ** -40)), np.float32(2.0 ** 40))
                top = max(top, want[j])
        assert T.bits(prio, want) and mx == top and prio.dtype == np.float32, (m, kind)
        ok = P._valid_rows(idx.astype(np.int64), val, C_)
        by_numpy = prio0.copy()
        by_numpy[idx[ok]] = np.clip(val[ok], np.float32(2.0 ** -40), np.float32(2.0 ** 40))        # NumPy's own rule for repeats
        assert T.bits(prio, by_numpy), (m, kind)
        set_leaves = prio[prio != prio0]
        assert ((set_leaves >= np.float32(2.0 ** -40)) & (set_leaves <= np.float32(2.0 ** 40))).all()
    # the range route across the wrap, without it, and the whole ring; max_prio is what the slots take and is not changed
    for start, n in ((0, 1), (C_ - 1, 1), (C_ // 2, C_ - C_ // 2), (C_ - 1, min(C_, 3)), (C_ // 3, C_)):
        prio, mx = P.set_reference(prio0, 7.5, start=start, n=n)
        want = prio0.copy()
        for i in range(n):
            want[(start + i) % C_] = 7.5
        assert T.bits(prio, want) and mx == np.float32(7.5)


# ---- 7: coarse proportionality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,base', [(0, 0), (1, 0), (2024, 5), (2 ** 63 + 11, 2 ** 40)])
def test_sample_reference_is_coarsely_proportional(seed, base):
    """2^16 draws at C = 1000, four blocks of 250 leaves with priorities 1, 2, 3, 4: the count in block b is, for independent draws,
    binomial(2^16, p_b) with p_b = 0.1 .. 0.4 — standard deviation sqrt(2^16 p_b (1 - p_b)) = 76.8, 102.4, 117.3, 125.4 — and must lie
    within 6 of them of 2^16 p_b.  Stratification only tightens this: one draw per stratum of width total / m puts every count within a
    few units of its expectation (seen: at most 1 off).  The seeds are fixed: the test is deterministic."""
    n = 1 << 16
    prio = np.repeat(np.array([1, 2, 3, 4], np.float32), 250)
    idx = P.sample_reference(prio, n, seed=seed, base=base)['index']
    share = np.array([0.1, 0.2, 0.3, 0.4])
    bar = 6 * np.sqrt(n * share * (1 - share))
    counts = np.bincount(idx // 250, minlength=4)
    print('seed %d base %d: block counts %s, expected %s, bars %s' % (seed, base, counts.tolist(), (n * share).tolist(), bar.round(1).tolist()))
    assert counts.sum() == n and (np.abs(counts - n * share) <= bar).all(), counts


# ---- 8: the weight and the new priority ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [1.0, 0.6])
@pytest.mark.parametrize('m', [1, 65, 4096])
def test_weigh_reference_against_float64(m, alpha):
    """w = (p_min / p)^beta and prio_new = (a + eps)^alpha in float64 on the same float32 inputs.  The bar: log_det and exp_det are each
    within 2 ulp of the float64 function (tests/test_math_det_host.py); |log p| <= 40 ln 2 = 27.8, so d = log p_min - log p carries at most
    (2 + 2 + 1) * 2^-24 * 55.5 = 1.7e-5 absolute, times beta <= 1 plus one rounding of the product (2^-24 * 55.5); exp turns an absolute
    error of its argument into a relative one of the result, plus its own 2 ulp: 2.1e-5 + 1.2e-7 < 2.5e-5 relative.  The same count holds
    for the new priority (|log s| is far smaller there)."""
    rows = T.weigh_rows(m, seed=int(alpha * 10), undrawn=m > 1)
    out = P.weigh_reference(beta=0.4, alpha=alpha, eps=1e-3, **rows)
    drawn = rows['index'] >= 0
    p64, pmin = rows['prio'].astype(np.float64), float(np.nanmin(rows['prio']))
    assert pmin == float(rows['min_partials'].min())
    w64 = np.where(drawn, (pmin / np.where(drawn, p64, 1.0)) ** float(np.float32(0.4)), 0.0)
    assert out['w'].dtype == np.float32 and (np.abs(out['w'] - w64) <= 2.5e-5 * w64).all()
    assert (out['w'] <= 1).all() and (out['w'][~drawn] == 0).all() and out['w'][np.nanargmin(rows['prio'])] == 1.0
    q1, q2, y = (rows[k].astype(np.float64) for k in ('q1', 'q2', 'y'))
    s64 = 0.5 * (np.abs(q1 - y) + np.abs(q2 - y)) + float(np.float32(1e-3))
    new64 = s64 ** float(np.float32(alpha))
    assert (np.abs(out['prio_new'][drawn] - new64[drawn]) <= 2.5e-5 * new64[drawn]).all() and np.isnan(out['prio_new'][~drawn]).all()
    for k in ('g_q1', 'g_q2', 'loss1', 'loss2'):
        assert T.bits(out[k], rows[k] * out['w'])                          # one rounding on top of eb_sac_critic's own
    one = P.weigh_reference(rows['index'], rows['prio'], rows['min_partials'], q1=rows['q1'], y=rows['y'], alpha=alpha, eps=1e-3)
    s1 = np.abs(q1 - y) + float(np.float32(1e-3))
    assert (np.abs(one['prio_new'][drawn] - (s1 ** float(np.float32(alpha)))[drawn]) <= 2.5e-5 * (s1 ** float(np.float32(alpha)))[drawn]).all()
    # beta from the counter: min(1, fmaf(step, counter, beta0)); a NaN TD error travels into prio_new and set_reference then skips it
    assert P.beta_reference(0.4, 0.01, 7) == np.float32(np.float64(np.float32(0.01)) * 7 + np.float64(np.float32(0.4)))
    assert P.beta_reference(0.4, 0.01, 700) == 1 and P.beta_reference(0.4) == np.float32(0.4)
    bad = T.weigh_rows(max(m, 12), nan=True)
    new = P.weigh_reference(alpha=alpha, **bad)['prio_new']
    assert np.isnan(new[::11]).all() and np.isnan(new[5::11]).all()
    prio, _ = P.set_reference(np.zeros(1000, np.float32), 1.0, index=bad['index'], value=new)
    touched = np.zeros(1000, bool)
    touched[bad['index'][~np.isnan(new)]] = True
    assert (prio[~touched] == 0).all() and (prio[touched] > 0).all()
