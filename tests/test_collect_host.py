"""CPU (-m "not gpu"): the collection family (include/envbuild_collect.h, env_build_amd.collect) — its header against the module's binding
table and argument structs, the separation of libenvbuild_collect.so from the other three libraries and the kernels its code object
holds, device-free refusals, the NumPy restatements against plain loops and float64 NumPy, and the truncation convention against the
textbook recursion."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import collect
from tests import _collect as T
from tests import _kernel_census as K
from tests._helpers import ROOT

STRUCTS = {'eb_collect_begin_args': collect.EbCollectBeginArgs, 'eb_collect_record_args': collect.EbCollectRecordArgs,
           'eb_collect_next_values_args': collect.EbCollectNextValuesArgs, 'eb_collect_episode_log_args': collect.EbCollectEpisodeLogArgs}


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(collect.COLLECT_PROTOTYPES) == sorted(T.ENTRIES + ('eb_collect_abi_version', 'eb_collect_last_error'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in STRUCTS.items()}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, args) in collect.COLLECT_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    assert not [n for n in names + list(T.KERNELS) if re.search(r'_gate(d|_|$)', n)]
    macros = {m: getattr(collect, m) for m in ('EB_COLLECT_ABI_VERSION', 'EB_COLLECT_LOG_BLOCKS', 'EB_COLLECT_LOG_FIELDS')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_COLLECT_\w+) ', text)) == sorted(macros)
    assert tuple(macros.values()) == (1, 64, 16)
    for name, struct in STRUCTS.items():
        assert T.struct_fields(src, name) == list(struct._fields_), name
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    assert collect.TIME_LIMIT == 7 == int(re.search(r'#define EB_DONE_TIME_LIMIT (\d+)', open(os.path.join(ROOT, 'include', 'envbuild.h')).read()).group(1))
    for words in ('ONE trunc_obs ROW PER ENV SUFFICES', 'max_episode_steps', 'AT CALL TIME', 'tests/test_stream_census.py', 't-major',
                  'libenvbuild_collect.so ONLY', 'eb_collect_last_error', 'record_reference', 'next_values_reference', 'episode_log_reference',
                  'is NOT touched', 'A select', 'sees no eb_mlp handle'):
        assert words in text, words


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import epoch, ppo, train
    others = set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES) | set(epoch.EPOCH_PROTOTYPES)
    assert not set(collect.COLLECT_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(collect.COLLECT_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in collect.__all__]


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_collect_sources_are_in_no_list_of_the_other_libraries():
    mine = set(T.UNIT) | {os.path.join('..', '..', 'include', 'envbuild_collect.h')}
    own = eb_build.COLLECT_SOURCES + eb_build.COLLECT_HEADERS
    assert eb_build.COLLECT_SOURCES == ['eb_collect.hip'] and mine <= set(own)
    others = [eb_build.SOURCES, eb_build.HEADERS, eb_build.TRAIN_SOURCES, eb_build.TRAIN_HEADERS, eb_build.EPOCH_SOURCES,
              eb_build.EPOCH_HEADERS] + list(eb_build.KERNEL_SOURCES.values())
    for files in others:
        assert not [f for f in files if 'collect' in f], files
    # the reverse: nothing of the other libraries but the return codes' header, read and never changed
    assert set(own) - mine == {os.path.join('..', '..', 'include', 'envbuild.h')}
    assert not [f for f in own + list(T.UNIT) + ['collect.py', 'test_collect_host.py', 'test_gpu_collect.py', '_collect.py'] if 'train' in f]
    assert eb_build.COLLECT_LIB not in (eb_build.LIB, eb_build.TRAIN_LIB, eb_build.EPOCH_LIB)
    assert os.path.dirname(eb_build.COLLECT_LIB) == os.path.dirname(eb_build.LIB) and os.path.basename(eb_build.COLLECT_LIB) == 'libenvbuild_collect.so'
    assert len({eb_build.collect_source_hash(), eb_build.epoch_source_hash(), eb_build.train_source_hash(), eb_build.source_hash()}) == 4
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_collect.hip']
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
    # no unit of the other libraries includes a collect header
    for f in eb_build.SOURCES + eb_build.HEADERS + eb_build.TRAIN_SOURCES + eb_build.TRAIN_HEADERS + eb_build.EPOCH_SOURCES + eb_build.EPOCH_HEADERS:
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            body = fh.read()
        assert 'eb_collect' not in body and 'envbuild_collect' not in body, f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly, nothing allocates, copies or synchronises
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence', 'hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in code, word
    assert '__syncthreads' in code and 'float4' in code and 'long long' in code


def test_the_code_object_holds_exactly_the_four_kernels():
    lib, blob = T.library()
    assert lib.eb_collect_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 26.'):]
    for k in T.KERNELS:
        assert k in section, k
    # the other three libraries export none of the entries and hold none of the kernels
    for path in (eb_build.build(), eb_build.build_train(), eb_build.build_epoch()):
        other = open(path, 'rb').read()
        for name in list(collect.COLLECT_PROTOTYPES) + list(T.KERNELS):
            assert name.encode() not in other, (path, name)


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    big = 2 ** 31 - 1

    def bargs(**kw):
        full = dict(n_env=4, obs_dim=3, obs=p, obs_buf=p, trunc_t=p)
        full.update(kw)
        return C.byref(collect.EbCollectBeginArgs(**full))

    record_pointers = ('obs', 'reward', 'ep_ret', 'ep_len', 'obs_buf', 'rew_buf', 'nonterminal', 'carry', 'ret_buf', 'len_buf')

    def rargs(**kw):
        full = dict(n_env=4, obs_dim=3, steps=2, t=0, done_code=p, code_buf=p, final_obs=p, trunc_obs=p, trunc_t=p)
        full.update({k: p for k in record_pointers})
        full.update(kw)
        return C.byref(collect.EbCollectRecordArgs(**full))

    def nargs(**kw):
        full = dict(n_env=4, steps=2, values=p, v_trunc=p, trunc_t=p, next_values=p)
        full.update(kw)
        return C.byref(collect.EbCollectNextValuesArgs(**full))

    def largs(**kw):
        full = dict(n_slots=8, ret_buf=p, len_buf=p, code_buf=p, out=p)
        full.update(kw)
        return C.byref(collect.EbCollectEpisodeLogArgs(**full))

    calls = [('eb_collect_begin', None), ('eb_collect_begin', bargs(n_env=-1)), ('eb_collect_begin', bargs(obs_dim=0)),
             ('eb_collect_begin', bargs(obs_dim=-3)), ('eb_collect_begin', bargs(n_env=big, obs_dim=2))]
    calls += [('eb_collect_begin', bargs(**{k: v})) for k in ('obs', 'obs_buf', 'trunc_t') for v in (None, p + 2)]
    calls += [('eb_collect_record', None), ('eb_collect_record', rargs(n_env=-1)), ('eb_collect_record', rargs(obs_dim=0)),
              ('eb_collect_record', rargs(steps=0)), ('eb_collect_record', rargs(steps=-1)), ('eb_collect_record', rargs(t=-1)),
              ('eb_collect_record', rargs(t=2)), ('eb_collect_record', rargs(n_env=big, obs_dim=2)),
              ('eb_collect_record', rargs(done_code=None)), ('eb_collect_record', rargs(code_buf=None)),
              ('eb_collect_record', rargs(final_obs=p + 2)), ('eb_collect_record', rargs(trunc_obs=None)),
              ('eb_collect_record', rargs(trunc_t=None)), ('eb_collect_record', rargs(trunc_obs=p + 1)),
              ('eb_collect_record', rargs(trunc_t=p + 2))]
    calls += [('eb_collect_record', rargs(**{k: v})) for k in record_pointers for v in (None, p + 2)]
    calls += [('eb_collect_next_values', None), ('eb_collect_next_values', nargs(n_env=-1)), ('eb_collect_next_values', nargs(steps=-1)),
              ('eb_collect_next_values', nargs(n_env=2 ** 30, steps=1))]
    calls += [('eb_collect_next_values', nargs(**{k: v})) for k in ('values', 'v_trunc', 'trunc_t', 'next_values') for v in (None, p + 2)]
    calls += [('eb_collect_episode_log', None), ('eb_collect_episode_log', largs(n_slots=-1)), ('eb_collect_episode_log', largs(n_slots=2 ** 31)),
              ('eb_collect_episode_log', largs(code_buf=None)), ('eb_collect_episode_log', largs(out=None)),
              ('eb_collect_episode_log', largs(out=p + 4))]
    calls += [('eb_collect_episode_log', largs(**{k: v})) for k in ('ret_buf', 'len_buf') for v in (None, p + 2)]
    assert len(calls) >= 60 and {name for name, _ in calls} == set(T.ENTRIES)
    for name, a in calls:
        assert getattr(lib, name)(a) == -1, name
        assert lib.eb_collect_last_error().startswith(name.encode() + b':'), (name, lib.eb_collect_last_error())
    assert all(v == 0.0 for v in buf)
    # no envs, no steps or no slots: a no-op that needs no pointer and no device
    nothing = dict(obs=None, obs_buf=None, trunc_t=None)
    assert lib.eb_collect_begin(bargs(n_env=0, **nothing)) == 0
    assert lib.eb_collect_record(rargs(n_env=0, done_code=None, code_buf=None, final_obs=None, trunc_obs=None, **dict(nothing, **{k: None for k in record_pointers}))) == 0
    assert lib.eb_collect_next_values(nargs(n_env=0, values=None, v_trunc=None, trunc_t=None, next_values=None)) == 0
    assert lib.eb_collect_next_values(nargs(steps=0, values=None, v_trunc=None, trunc_t=None, next_values=None)) == 0
    assert lib.eb_collect_episode_log(largs(n_slots=0, ret_buf=None, len_buf=None, code_buf=None, out=None)) == 0
    assert all(v == 0.0 for v in buf)


# ---- 4: record_reference against a plain loop ------------------------------------------------------------------------------------------------
HAND_CODES = np.array([[0, 1, 0, 7, 0, 7],          # [T, B]: every code 0 .. 7 appears; envs 3 and 5 are truncated (at steps 0 and 3);
                       [2, 0, 3, 0, 0, 0],          # env 0 finishes twice (steps 1 and 3); env 4 never finishes
                       [0, 4, 0, 5, 0, 0],
                       [6, 0, 0, 0, 0, 7]], np.uint8)


def plain_loop(codes, obs0, obs, reward, final, with_final):
    """the header's per-env rules, one env and one step at a time, in Python"""
    Tn, B = codes.shape
    D = obs0.shape[1]
    buf = T.sentinel_buffers(Tn, B, D)
    for i in range(B):
        buf['obs_buf'][0, i] = obs0[i]
        buf['trunc_t'][i] = -1
    for t in range(Tn):
        for i in range(B):
            c = int(codes[t, i])
            live, trunc = c == 0, c == 7 and with_final
            for d in range(D):
                buf['obs_buf'][t + 1, i, d] = obs[t, i, d]
            buf['rew_buf'][t, i] = reward[t, i]
            buf['nonterminal'][t, i] = 1.0 if (live or trunc) else 0.0
            buf['carry'][t, i] = 1.0 if live else 0.0
            if trunc:
                buf['trunc_obs'][i] = final[t, i]
                buf['trunc_t'][i] = t
            R = np.float32(buf['ep_ret'][i]) + np.float32(reward[t, i])
            L = int(buf['ep_len'][i]) + 1
            buf['ret_buf'][t, i], buf['len_buf'][t, i], buf['code_buf'][t, i] = R, L, c
            buf['ep_ret'][i], buf['ep_len'][i] = (0.0, 0) if c != 0 else (R, L)
    return buf


@pytest.mark.parametrize('with_final', [True, False])
def test_record_reference_against_a_plain_loop(with_final):
    Tn, B, D = HAND_CODES.shape[0], HAND_CODES.shape[1], 3
    assert set(HAND_CODES.ravel()) == set(range(8))
    rng = np.random.default_rng(5)
    obs0, obs = rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((Tn, B, D)).astype(np.float32)
    reward, final = rng.standard_normal((Tn, B)).astype(np.float32), rng.standard_normal((Tn, B, D)).astype(np.float32)
    want = plain_loop(HAND_CODES, obs0, obs, reward, final, with_final)
    got = collect.begin_reference(T.sentinel_buffers(Tn, B, D), obs0)
    for t in range(Tn):
        assert collect.record_reference(got, t, obs[t], reward[t], HAND_CODES[t], final[t] if with_final else None) is got
    assert sorted(got) == sorted(k for k, _ in collect.BUFFERS)
    for k in got:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # what the case is there to show
    assert got['trunc_t'].tolist() == ([-1, -1, -1, 0, -1, 3] if with_final else [-1] * B)
    untouched = got['trunc_t'] < 0
    assert (got['trunc_obs'][untouched] == T.SENTINEL).all()                 # a row of an env that is not truncated is not touched
    if with_final:
        assert np.array_equal(got['trunc_obs'][3], final[0, 3]) and np.array_equal(got['trunc_obs'][5], final[3, 5])
        assert got['nonterminal'][0, 3] == 1.0 and got['carry'][0, 3] == 0.0
    else:
        assert got['nonterminal'][0, 3] == 0.0 and got['carry'][0, 3] == 0.0
    assert got['len_buf'][:, 0].tolist() == [1, 2, 1, 2] and got['len_buf'][:, 4].tolist() == [1, 2, 3, 4]   # env 0 finishes twice
    assert got['ep_len'].tolist() == [0, 1, 2, 1, 4, 0]
    assert got['ret_buf'][3, 4] == np.float32(np.float32(np.float32(reward[0, 4] + reward[1, 4]) + reward[2, 4]) + reward[3, 4])
    with pytest.raises(ValueError):
        collect.record_reference(got, Tn, obs[0], reward[0], HAND_CODES[0])


# ---- 5: next_values_reference -------------------------------------------------------------------------------------------------------------------
def test_next_values_reference_is_a_select():
    Tn, B = 3, 4
    rng = np.random.default_rng(6)
    values = rng.standard_normal((Tn + 1, B)).astype(np.float32)
    trunc_t = np.array([-1, 0, Tn - 1, -1], np.int32)
    v_trunc = np.array([np.nan, 10.0, 20.0, np.nan], np.float32)            # the rows of envs 0 and 3 are unused: their NaN must not travel
    got = collect.next_values_reference(values, v_trunc, trunc_t)
    want = values[1:].copy()
    want[0, 1], want[Tn - 1, 2] = 10.0, 20.0
    assert got.dtype == np.float32 and np.array_equal(got, want) and not np.isnan(got).any()
    # T = 1: the one row is values[1] or v_trunc
    got = collect.next_values_reference(values[:2], v_trunc, np.array([-1, 0, 2, -1], np.int32))
    assert np.array_equal(got, np.array([[values[1, 0], 10.0, values[1, 2], values[1, 3]]], np.float32))


# ---- 6: the episode log's restatement ----------------------------------------------------------------------------------------------------------
def log_inputs(n, finished, seed=0):
    """ret, len, code of n slots; finished: 'none', 'all' or 'some'"""
    rng = np.random.default_rng(seed + n)
    ret = (3.0 + 20.0 * rng.standard_normal(n)).astype(np.float32)
    length = rng.integers(1, 200, n).astype(np.int32)
    code = {'none': np.zeros(n, np.int64), 'all': rng.integers(1, 8, n), 'some': rng.integers(0, 8, n) * (rng.random(n) < 0.3)}[finished]
    return ret, length, code.astype(np.uint8)


@pytest.mark.parametrize('finished', ['none', 'all', 'some'])
@pytest.mark.parametrize('n', [1, 255, 257, 16385, 40000])
def test_episode_log_reference_and_fold_against_float64_numpy(n, finished):
    """counts, maximum and minimum exact; the means within 1e-12 of sum |x| / n (DESIGN.md §25's bar for the same fold); the variance
    within 2e-12 of mean R^2: its two terms, mean R^2 and (mean R)^2 <= mean R^2, each carry the bar of a mean"""
    ret, length, code = log_inputs(n, finished)
    blocks = collect.episode_log_reference(ret, length, code)
    assert blocks.shape == (64, 16) and blocks.dtype == np.float64
    got = collect.fold_episode_log(blocks)
    done = code != 0
    m = int(done.sum())
    assert got['episodes'] == m and got['slots'] == n and got['nonfinite'] == 0
    assert got['outcomes'] == {name: int((code == k).sum()) for k, name in enumerate(_capi.DONE_NAMES)}
    assert list(got['outcomes']) == list(_capi.DONE_NAMES)
    assert np.array_equal(blocks[:, 15], np.bincount((np.arange(n) % 16384) // 256, minlength=64))          # the kernel's cut of the slots
    if m == 0:
        assert all(np.isnan(got[k]) for k in ('return_mean', 'return_std', 'length_mean', 'return_max', 'return_min'))
        assert (blocks[:, 4] == -np.inf).all() and (blocks[:, 5] == np.inf).all() and (blocks[:, :4] == 0.0).all()
        return
    R, Ln = ret[done].astype(np.float64), length[done].astype(np.float64)
    assert got['return_max'] == R.max() and got['return_min'] == R.min()
    assert abs(got['return_mean'] - R.mean()) <= 1e-12 * np.abs(R).sum() / m
    assert abs(got['length_mean'] - Ln.mean()) <= 1e-12 * Ln.sum() / m
    assert abs(got['return_std'] ** 2 - R.var()) <= 2e-12 * (R * R).sum() / m
    empty = blocks[:, 0] == 0
    assert (blocks[empty, 4] == -np.inf).all() and (blocks[empty, 5] == np.inf).all()


def test_episode_log_reference_with_bad_returns():
    n = 600
    ret, length, code = log_inputs(n, 'all')
    ret[5], ret[300], ret[599] = np.nan, np.inf, np.nan
    code[7] = 0
    ret[7] = np.nan                                                       # not finished: its return is never looked at
    blocks = collect.episode_log_reference(ret, length, code)
    got = collect.fold_episode_log(blocks)
    assert got['episodes'] == n - 1 and got['nonfinite'] == 3 and blocks[0, 6] == 1 and blocks[1, 6] == 1 and blocks[2, 6] == 1
    assert got['return_max'] == np.inf and got['return_mean'] == np.inf       # an infinity is in the sums and in the maximum: IEEE
    ok = np.isfinite(ret) & (code != 0)
    assert got['return_min'] == ret[ok].min() and got['length_mean'] == length[code != 0].astype(np.float64).sum() / (n - 1)
    # NaNs alone: passed over by the sums, the maximum and the minimum
    ret[300] = 1.0
    ok = np.isfinite(ret) & (code != 0)
    got = collect.fold_episode_log(collect.episode_log_reference(ret, length, code))
    R = ret[ok].astype(np.float64)
    assert got['nonfinite'] == 2 and got['return_max'] == R.max() and got['return_min'] == R.min()
    assert abs(got['return_mean'] - R.sum() / (n - 1)) <= 1e-12 * np.abs(R).sum() / (n - 1)
    with pytest.raises(ValueError):
        collect.fold_episode_log(np.zeros((64, 8)))
    with pytest.raises(ValueError):
        collect.episode_log_reference(ret, length[:-1], code)


# ---- 7: the truncation convention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_truncation_bootstraps_from_the_final_observation(dtype):
    """3 steps x 2 envs.  Env 0 is truncated by the time limit at step 1 and starts a new episode at step 2; env 1 collides at step 0.
    The textbook: delta_t = r_t + gamma * V(next state of t) - V(s_t), where the next state of a truncated step is its FINAL observation and
    a terminated step has none; A_t = delta_t + gamma * lam * A_{t+1} inside an episode, A_t = delta_t at its last step.  Written out in
    the operation order of eb_gae, so the comparison is bit for bit in both precisions."""
    from env_build_amd.ppo import gae_reference
    f = dtype
    Tn, B, D = 3, 2, 2
    gamma, lam = 0.9, 0.8
    codes = np.array([[0, 1], [7, 0], [0, 0]], np.uint8)
    r = np.array([[1.0, -2.0], [0.5, 0.25], [-1.5, 3.0]], np.float32)
    V = np.array([[0.7, 1.1], [0.3, -0.4], [2.0, 0.6], [1.3, -0.9]], np.float32)        # [T + 1, B]: the last row is v_last
    v_final = np.float32(5.5)                                                        # V(final observation of env 0 at step 1)
    buf = collect.begin_reference(collect.buffers(Tn, B, D), np.zeros((B, D), np.float32))
    final = np.full((B, D), 9.0, np.float32)
    for t in range(Tn):
        collect.record_reference(buf, t, np.zeros((B, D), np.float32), r[t], codes[t], final)
    assert buf['trunc_t'].tolist() == [1, -1] and (buf['trunc_obs'][0] == 9.0).all()
    nv = collect.next_values_reference(V, np.array([v_final, np.nan], np.float32), buf['trunc_t'])
    adv, ret = gae_reference(buf['rew_buf'], V[:Tn], None, buf['nonterminal'], gamma, lam, next_values=nv, carry=buf['carry'], dtype=dtype)
    g, gl = f(gamma), f(gamma * lam)
    r_, V_ = r.astype(f), V.astype(f)
    want = np.zeros((Tn, B), f)
    # env 0: episode one is steps 0 and 1 (truncated), episode two starts at step 2 and is still running at the end
    want[2, 0] = (r_[2, 0] + g * V_[3, 0]) - V_[2, 0]
    want[1, 0] = (r_[1, 0] + g * f(v_final)) - V_[1, 0]
    want[0, 0] = ((r_[0, 0] + g * V_[1, 0]) - V_[0, 0]) + gl * want[1, 0]
    # env 1: the collision at step 0 ends an episode with no bootstrap; steps 1 and 2 belong to the next one
    want[2, 1] = (r_[2, 1] + g * V_[3, 1]) - V_[2, 1]
    want[1, 1] = ((r_[1, 1] + g * V_[2, 1]) - V_[1, 1]) + gl * want[2, 1]
    want[0, 1] = r_[0, 1] - V_[0, 1]
    assert adv.dtype == f and np.array_equal(adv, want), (adv, want)
    assert np.array_equal(ret, adv + V_[:Tn])
    # an implementation that treats the truncation as a termination gives another number at the truncated step and before it
    plain, _ = gae_reference(buf['rew_buf'], V[:Tn], V[Tn], (codes == 0).astype(np.float32), gamma, lam, dtype=dtype)
    assert plain[1, 0] == r_[1, 0] - V_[1, 0] and plain[1, 0] != adv[1, 0] and plain[0, 0] != adv[0, 0]
    assert np.array_equal(plain[2], adv[2]) and np.array_equal(plain[:, 1], adv[:, 1])
