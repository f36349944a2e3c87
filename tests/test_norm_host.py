"""CPU (-m "not gpu"): the normalisation family (include/envbuild_norm.h, env_build_amd.norm) — its header against the module's binding
table and argument structs, the separation of libenvbuild_norm.so from the other six libraries and the kernels its code object holds,
device-free refusals, the NumPy restatements against a float64 evaluation of the same formulas under the derived bars, fixture G22 under
the triangle bar, and the edge cases of the state: a constant column, a poisoned column, the parameter round trips."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import norm
from tests import _kernel_census as K
from tests import _norm as T
from tests._helpers import ROOT

STRUCTS = {'eb_norm_update_args': norm.EbNormUpdateArgs, 'eb_norm_apply_args': norm.EbNormApplyArgs}
OTHERS = ('', 'train_', 'epoch_', 'collect_', 'ctl_', 'ac_')


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(norm.NORM_PROTOTYPES) == sorted(T.ENTRIES + ('eb_norm_abi_version', 'eb_norm_last_error', 'eb_norm_workspace_bytes'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in STRUCTS.items()}
    kinds['int32_t'] = C.c_int32
    results = {'int': C.c_int, 'const char*': C.c_char_p, 'size_t': C.c_size_t}
    for name, (res, args) in norm.NORM_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*|\bsize_t)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    macros = {m: getattr(norm, m) for m in ('EB_NORM_ABI_VERSION', 'EB_NORM_MAX_DIM', 'EB_NORM_MAX_BLOCKS')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_NORM_\w+) ', text)) == sorted(macros) and tuple(macros.values()) == (1, 256, 512)
    for name, struct in STRUCTS.items():
        assert T.struct_fields(src, name) == list(struct._fields_), name
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    for words in ('libenvbuild_norm.so ONLY', 'eb_norm_last_error', 'AT CALL TIME', 'tests/test_stream_census.py', 'exactly TWO launches',
                  'ONE launch', 'NEVER writes', 'RAISES as written', 'np.zeros', 'update_reference', 'apply_reference', 'a NaN travels',
                  'neither read nor written', 'pure function of (n, D)', 'count 1e-4', 'BEFORE the launch'):
        assert words in text, words


def test_the_capture_test_holds_both_entries_as_the_struct_census_asks():
    """tests/_capture_cases.py's table of struct-taking entries (STRUCT_STREAM_HELD) is a fixed list of the other families' twenty; the
    header declares these two prototypes without a parameter name, as envbuild_ac.h does, which that parser passes over.  The obligation
    itself is applied here, with the census's own function_text: the named GPU test mentions the entry, runs it on a side stream, captures
    and replays it."""
    from tests._capture_cases import STRUCT_STREAM_HELD, function_text, stream_entries, struct_stream_entries
    _, src = T.header()
    for entry, struct in (('eb_norm_update', 'eb_norm_update_args'), ('eb_norm_apply', 'eb_norm_apply_args')):
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*\)\s*;' % (entry, struct), src), entry
        assert ('stream', C.c_void_p) in T.struct_fields(src, struct)
        assert entry not in STRUCT_STREAM_HELD and entry not in struct_stream_entries() and entry not in stream_entries()
        text = function_text('test_gpu_norm', 'test_every_entry_on_a_side_stream_and_under_capture')
        assert text is not None and re.search(r"['\"]%s['\"]" % entry, text), entry
        assert 'side' in text and re.search(r'\bcapture\(', text) and 'replay' in text, entry
    assert len(struct_stream_entries()) == 20 and len(stream_entries()) == 50


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import ac, collect, ctl, epoch, ppo, train
    others = (set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES) | set(epoch.EPOCH_PROTOTYPES)
              | set(collect.COLLECT_PROTOTYPES) | set(ctl.CTL_PROTOTYPES) | set(ac.AC_PROTOTYPES))
    assert not set(norm.NORM_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(norm.NORM_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in norm.__all__]


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_norm_sources_are_in_no_list_of_the_other_libraries():
    header = os.path.join('..', '..', 'include', 'envbuild_norm.h')
    mine = set(T.UNIT) | {header}
    own = eb_build.NORM_SOURCES + eb_build.NORM_HEADERS
    assert eb_build.NORM_SOURCES == ['eb_norm.hip'] and mine <= set(own)
    lists = [getattr(eb_build, (p.upper() + kind)) for p in OTHERS for kind in ('SOURCES', 'HEADERS')]
    for files in lists + list(eb_build.KERNEL_SOURCES.values()):
        assert not [f for f in files if 'norm' in f], files
    assert set(own) - mine == {os.path.join('..', '..', 'include', 'envbuild.h')}          # the return codes' header, read and never changed
    libs = [getattr(eb_build, p.upper() + 'LIB') for p in OTHERS]
    assert eb_build.NORM_LIB not in libs and os.path.dirname(eb_build.NORM_LIB) == os.path.dirname(eb_build.LIB)
    assert os.path.basename(eb_build.NORM_LIB) == 'libenvbuild_norm.so'
    hashes = {getattr(eb_build, p + 'source_hash')() for p in OTHERS} | {eb_build.norm_source_hash()}
    assert len(hashes) == 7
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_norm.hip']
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
    # no unit of the other libraries includes a norm header
    for files in lists:
        for f in files:
            with open(os.path.join(eb_build.CSRC, f)) as fh:
                body = fh.read()
            assert 'eb_norm' not in body and 'envbuild_norm' not in body, f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly, nothing allocates, copies or synchronises
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence', 'hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in code, word
    assert '__syncthreads' in code and 'float4' in code and 'long long' in code
    # the build entry compiles it; the smoke run is as it was
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '_b.build_norm()' in entry and 'norm' not in entry[entry.index('def smoke'):]


def test_the_code_object_holds_exactly_the_three_kernels():
    lib, blob = T.library()
    assert lib.eb_norm_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 29.'):]
    for k in T.KERNELS:
        assert k in section, k
    for D in (0, 1, 41, 256, 257, -1):
        assert lib.eb_norm_workspace_bytes(D) == norm.workspace_bytes(D)
    assert norm.workspace_bytes(41) == 512 * 2 * 42 * 8 and norm.workspace_bytes(257) == 0


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    big, nan, inf = 2 ** 31 - 1, float('nan'), float('inf')
    update_pointers = ('x', 'obs_stat', 'obs_scale', 'reward', 'ret_run', 'ret_stat', 'ret_scale', 'workspace')
    apply_pointers = ('obs_scale', 'x', 'y', 'sel_x', 'sel', 'ret_scale', 'reward', 'reward_out', 'done_code', 'ret_run')

    def uargs(**kw):
        full = dict(n=4, dim=3, gamma=0.99, eps=1e-8, **{k: p for k in update_pointers})
        full.update(kw)
        return C.byref(norm.EbNormUpdateArgs(**full))

    def aargs(**kw):
        full = dict(n=4, dim=3, sel_value=1, clip_obs=10.0, clip_rew=10.0, **{k: p for k in apply_pointers})
        full.update(kw)
        return C.byref(norm.EbNormApplyArgs(**full))

    U, A = 'eb_norm_update', 'eb_norm_apply'
    calls = [(U, None), (U, uargs(n=-1)), (U, uargs(dim=0)), (U, uargs(dim=257)), (U, uargs(dim=-1)), (U, uargs(n=big, dim=2)),
             (U, uargs(gamma=nan)), (U, uargs(gamma=inf)), (U, uargs(eps=nan)), (U, uargs(eps=-inf)), (U, uargs(x=None, reward=None)),
             (U, uargs(x=p + 2)), (U, uargs(reward=p + 2)), (U, uargs(obs_stat=p + 4)), (U, uargs(ret_stat=p + 4)), (U, uargs(workspace=p + 4))]
    calls += [(U, uargs(**{k: v})) for k in ('obs_stat', 'obs_scale', 'ret_run', 'ret_stat', 'ret_scale', 'workspace') for v in (None, p + 2)]
    calls += [(A, None), (A, aargs(n=-1)), (A, aargs(dim=0)), (A, aargs(dim=257)), (A, aargs(n=big, dim=2)), (A, aargs(clip_obs=nan)),
              (A, aargs(clip_obs=inf)), (A, aargs(clip_rew=nan)), (A, aargs(clip_rew=-inf)), (A, aargs(x=None, sel_x=None, reward=None)),
              (A, aargs(x=p + 2)), (A, aargs(sel_x=p + 2)), (A, aargs(reward=p + 2)), (A, aargs(done_code=None)), (A, aargs(ret_run=None)),
              (A, aargs(ret_run=p + 2)), (A, aargs(reward=None))]
    calls += [(A, aargs(**{k: v})) for k in ('obs_scale', 'y', 'sel', 'ret_scale', 'reward_out') for v in (None, p + 2)]
    assert len(calls) >= 50 and {name for name, _ in calls} == set(T.ENTRIES)
    for k, (name, a) in enumerate(calls):
        assert getattr(lib, name)(a) == -1, (k, name)
        assert lib.eb_norm_last_error().startswith(name.encode() + b':'), (name, lib.eb_norm_last_error())
    assert all(v == 0.0 for v in buf)
    # no rows: a no-op that needs no pointer and no device
    assert lib.eb_norm_update(uargs(n=0, **{k: None for k in update_pointers})) == 0
    assert lib.eb_norm_apply(aargs(n=0, **{k: None for k in apply_pointers})) == 0
    assert all(v == 0.0 for v in buf)
    # the module's own refusals
    with pytest.raises(ValueError):
        norm.HostState(0)
    with pytest.raises(ValueError):
        norm.HostState(257)
    with pytest.raises(ValueError):
        norm.HostState(3).set_params(np.zeros(2), np.ones(3), 1.0)


# ---- 4: the restatements against float64 -------------------------------------------------------------------------------------------------------
SWEEP_WORST = {}


@pytest.mark.parametrize('D', [1, 41, 137])
@pytest.mark.parametrize('B', [2, 7, 65, 257, 1000])
def test_restatements_against_float64_under_the_derived_bar(B, D):
    """four consecutive updates, |mean| <= 10^3, std from 0 to 10^2: |y - y64| <= 2^-23 (|mean| / den + 4 |y64|) elementwise (tests/_norm.py:
    obs_bar).  Worst ratio seen over the sweep: 0.49."""
    state, s64 = norm.HostState(D), T.State64(D)
    worst = 0.0
    for k in range(4):
        x = T.sweep_batch(B, D, k)
        assert norm.update_reference(state, x) is state
        s64.update(x)
        y, y64 = norm.apply_reference(state, x, 10.0), s64.apply(x, 10.0)
        bar = T.obs_bar(s64.mean, s64.den, y64)
        err = np.abs(y.astype(np.float64) - y64)
        assert y.dtype == np.float32 and y.shape == x.shape and (err <= bar).all(), (k, float((err / bar).max()))
        worst = max(worst, float((err / bar).max()))
        assert state.stat[2 * D] == s64.count
        assert np.array_equal(state.scale, norm._scale_of(state.stat[:D], state.stat[D:2 * D], state.eps_f))
    SWEEP_WORST[(B, D)] = worst
    print('B %d D %d: worst |y - y64| / bar = %.3f' % (B, D, worst))
    assert (state.stat[D:2 * D] >= 0.0).all()


@pytest.mark.parametrize('B', [1, 65, 1000])
def test_return_restatement_against_float64(B):
    """5 steps of process_rew with done codes.  The running return is the contract's own fp32 recursion — one fp32 multiply, one fp32 add,
    the reference's on float32 rewards — and is shared by both sides; the statistics and the division are held to float64 under
    |r - r64| <= 2^-23 * 4 |r64|."""
    rng = np.random.default_rng(B)
    state, s64 = norm.HostState(1), T.State64(1)
    ret_run = np.zeros(B, np.float32)
    for t in range(5):
        reward = (-3.0 + 40.0 * rng.standard_normal(B)).astype(np.float32)
        done = (np.arange(B) + t) % 8
        before = ret_run.copy()
        norm.update_return_reference(state, reward, ret_run, 0.99)
        assert np.array_equal(ret_run, (before * np.float32(0.99)).astype(np.float32) + reward)
        s64.update(ret_run.astype(np.float64))
        held = ret_run.copy()
        r = norm.apply_reward_reference(state, reward, 10.0, done, ret_run)
        r64 = s64.apply_reward(reward, 10.0)
        assert r.dtype == np.float32 and (np.abs(r.astype(np.float64) - r64) <= T.rew_bar(r64)).all(), t
        assert np.array_equal(ret_run, np.where(done != 0, np.float32(0), held))
    assert state.stat[2] == s64.count


def test_partial_sums_order_is_the_kernels():
    """the restated order against a plain loop over blocks, lanes and rows at a shape with two passes, a partial run and G = 6"""
    n, D = 512 * 32 + 45, 41
    rng = np.random.default_rng(3)
    x = (5.0 + rng.standard_normal((n, D))).astype(np.float32)
    K = rng.standard_normal(D)
    S1, S2 = norm.partial_sums_reference(x, K)
    G, blocks = 6, 512
    d = 7                                                                    # one column, by hand
    total1 = total2 = 0.0
    for b in range(blocks):
        lane1, lane2 = [0.0] * G, [0.0] * G
        for row0 in range(32 * b, n, 32 * blocks):
            for g in range(G):
                for r in range(g, min(32, n - row0), G):
                    v = float(x[row0 + r, d]) - K[d]
                    lane1[g] += v
                    lane2[g] += v * v
        for w in (4, 2, 1):
            for g in range(w):
                if g + w < G:
                    lane1[g] += lane1[g + w]
                    lane2[g] += lane2[g + w]
        total1 += lane1[0]
        total2 += lane2[0]
    assert S1[d] == total1 and S2[d] == total2
    assert norm._groups(1) == 32 and norm._groups(41) == 6 and norm._groups(137) == 1 and norm._groups(256) == 1 and norm._groups(8) == 32


# ---- 5: fixture G22 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 41])
@pytest.mark.parametrize('B', [2, 65])
def test_g22_observations_under_the_triangle_bar(B, D):
    """|y - y_ref| <= |y_ref - y64| + 2^-23 (|mean| / den + 4 |y64|), elementwise, from the fixture's own y_ref and y64"""
    g = T.golden()
    key = 'obs_B%d_D%d/' % (B, D)
    assert g[key + 'x'].shape == (6, B, D) and g[key + 'y_ref'].dtype == np.float32 and g[key + 'y64'].dtype == np.float64
    clip = float(g[key + 'clip'])
    at = np.abs(g[key + 'y64']) >= clip
    assert at.mean() <= 0.25 and (~at).reshape(-1, D).any(axis=0).all() and (B < 8 or at.any())
    print('G22 %s worst |y - y_ref| / bar = %.3f; the reference itself sits at %.1f x obs_bar from float64'
          % (key, T.replay_obs(T.HostEngine(), B, D),
             float((np.abs(g[key + 'y_ref'] - g[key + 'y64']) / np.maximum(T.obs_bar(g[key + 'mean_64'], np.sqrt(g[key + 'var_64'] + 1e-8), g[key + 'y64']), 1e-300)).max())))


@pytest.mark.parametrize('which', ['rew1', 'rewB'])
def test_g22_rewards_under_the_triangle_bar(which):
    g = T.golden()
    assert g['rew1/rew'].shape == (40,) and int(g['rew1/done'].sum()) == 3 and g['rewB/rew'].shape == (6, 65)
    assert set(np.unique(g['rewB/done'])) > {0, 1}
    print('G22 %s worst |r - r_ref| / bar = %.3f' % (which, T.replay_rewards(T.HostEngine(), which)))


def test_g22_holds_arrays_and_names_only():
    assert os.path.getsize(T.GOLD) < (1 << 20)
    z = np.load(T.GOLD, allow_pickle=False)
    assert len(z.files) == 56 and all(z[k].dtype.kind in 'fu' for k in z.files)


# ---- 6: the state's edge cases -------------------------------------------------------------------------------------------------------------------
def test_a_constant_column_gives_a_variance_of_at_least_zero_and_a_finite_output():
    for value in (0.0, 3.25, -1234.5678, 1e-30, 1e18):                    # (1e18: its square is still a float32)
        state = norm.HostState(2)
        for k in range(4):
            x = np.full((65, 2), value, np.float32)
            x[:, 1] = np.random.default_rng(k).standard_normal(65)
            norm.update_reference(state, x)
            y = norm.apply_reference(state, x, 10.0)
            var = state.stat[2:4]
            assert (var >= 0.0).all() and np.isfinite(state.scale).all() and (state.scale[2:] > 0).all(), (value, k, var)
            assert np.isfinite(y).all() and (np.abs(y) <= 10.0).all(), (value, k)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_a_bad_observation_poisons_only_its_own_column(bad):
    B, D = 65, 41
    clean, dirty = norm.HostState(D), norm.HostState(D)
    for k in range(3):
        x = T.sweep_batch(B, D, k, spread=False)
        xb = x.copy()
        if k == 1:
            xb[17, 5] = bad
        norm.update_reference(clean, x)
        norm.update_reference(dirty, xb)
        y, yb = norm.apply_reference(clean, x, 10.0), norm.apply_reference(dirty, xb, 10.0)
        others = np.arange(D) != 5
        assert np.array_equal(y[:, others], yb[:, others]), k
        assert np.array_equal(clean.stat[:2 * D].reshape(2, D)[:, others], dirty.stat[:2 * D].reshape(2, D)[:, others])
        assert np.array_equal(clean.scale.reshape(2, D)[:, others], dirty.scale.reshape(2, D)[:, others]) and clean.stat[2 * D] == dirty.stat[2 * D]
        if k >= 1:
            assert not np.isfinite(dirty.stat[[5, D + 5]]).all() and np.isnan(yb[:, 5]).all()        # it travels, and stays in its column


def test_parameters_round_trip(tmp_path):
    D = 41
    state = norm.HostState(D)
    for k in range(2):
        norm.update_reference(state, T.sweep_batch(65, D, k))
    again = norm.HostState(D)
    again.set_params(*state.get_params())
    assert np.array_equal(again.scale.view(np.uint32), state.scale.view(np.uint32)) and np.array_equal(again.stat, state.stat)
    mean, var, count = state.get_params()
    assert mean.dtype == var.dtype == np.float64 and mean.shape == var.shape == (D,) and abs(count - (130 + 1e-4)) < 1e-9
    first = norm.HostState(D)
    assert first.get_params()[2] == 1e-4 and (first.stat[:D] == 0).all() and (first.stat[D:2 * D] == 1).all()
    assert np.array_equal(first.scale[D:], np.full(D, np.sqrt(np.float32(1) + np.float32(1e-8)), np.float32))
    # the reference's ppc_params.npy: np.save of the dict get_params() returns (preprocessor.py:176-182), float32 arrays
    ret = (np.float32(-2.5), np.float32(31.0), 77.0001)
    params = {'ob_rms': (mean.astype(np.float32), var.astype(np.float32), count), 'ret_rms': ret}
    np.save(str(tmp_path / 'ppc_params.npy'), params)
    back = norm._read_params(str(tmp_path / 'ppc_params.npy'))
    assert sorted(back) == ['ob_rms', 'ret_rms']
    loaded = norm.HostState(D)
    loaded.set_params(*back['ob_rms'])
    assert np.array_equal(loaded.stat[:D], mean.astype(np.float32).astype(np.float64)) and loaded.stat[2 * D] == count
    one = norm.HostState(1)
    one.set_params(*back['ret_rms'])
    assert one.get_params() == (np.array([-2.5]), np.array([31.0]), 77.0001)
    # the module's own .npz
    np.savez(str(tmp_path / 'ppc_params.npz'), ob_rms_mean=mean, ob_rms_var=var, ob_rms_count=np.float64(count))
    back = norm._read_params(str(tmp_path / 'ppc_params.npz'))
    assert sorted(back) == ['ob_rms'] and np.array_equal(back['ob_rms'][0], mean) and back['ob_rms'][2] == count
