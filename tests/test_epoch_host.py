"""CPU (-m "not gpu"): the epoch family (include/envbuild_epoch.h, env_build_amd.epoch) — its header against the module's binding table
and argument structs, the separation of libenvbuild_epoch.so from the other two libraries and the kernels its code object holds,
device-free refusals, the index function's restatement as a bijection with the coarse uniformity the header promises, and the NumPy
restatements of the statistics and of the log against NumPy / torch float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import epoch
from tests import _epoch as T
from tests import _kernel_census as K
from tests._helpers import ROOT


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(epoch.EPOCH_PROTOTYPES) == sorted(T.ENTRIES + ('eb_epoch_abi_version', 'eb_epoch_last_error'))
    kinds = {'const eb_gather_args*': C.POINTER(epoch.EbGatherArgs), 'const eb_adv_stats_args*': C.POINTER(epoch.EbAdvStatsArgs),
             'const eb_ppo_log_args*': C.POINTER(epoch.EbPpoLogArgs), 'const eb_epoch_advance_args*': C.POINTER(epoch.EbEpochAdvanceArgs)}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, args) in epoch.EPOCH_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    assert not [n for n in names + list(T.KERNELS) if re.search(r'_gate(d|_|$)', n)]
    macros = {m: getattr(epoch, m) for m in ('EB_EPOCH_ABI_VERSION', 'EB_EPOCH_MAX_SOURCES', 'EB_EPOCH_MAX_WIDTH', 'EB_EPOCH_GATHER_ROWS',
                                             'EB_EPOCH_PARTIALS', 'EB_EPOCH_LOG_BLOCKS', 'EB_EPOCH_LOG_FIELDS')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_EPOCH_\w+) ', text)) == sorted(macros)
    assert (macros['EB_EPOCH_ABI_VERSION'], macros['EB_EPOCH_PARTIALS'], macros['EB_EPOCH_LOG_BLOCKS'], macros['EB_EPOCH_MAX_SOURCES']) == (1, 256, 64, 8)
    assert T.struct_fields(src, 'eb_gather_source') == list(epoch.EbGatherSource._fields_)
    assert T.struct_fields(src, 'eb_gather_args', {'eb_gather_source': epoch.EbGatherSource}, macros) == list(epoch.EbGatherArgs._fields_)
    assert T.struct_fields(src, 'eb_adv_stats_args') == list(epoch.EbAdvStatsArgs._fields_)
    assert T.struct_fields(src, 'eb_ppo_log_args') == list(epoch.EbPpoLogArgs._fields_)
    assert T.struct_fields(src, 'eb_epoch_advance_args') == list(epoch.EbEpochAdvanceArgs._fields_)
    for struct in (epoch.EbGatherArgs, epoch.EbAdvStatsArgs, epoch.EbPpoLogArgs, epoch.EbEpochAdvanceArgs):
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    for words in ('KEYED BIJECTION', 'NOT a certified uniform shuffle', 'AT CALL TIME', 'tests/test_stream_census.py', 'ALWAYS exactly TWO launches',
                  'pure function of n', 'LOSES DIGITS', 'NEVER dereferenced', 'libenvbuild_epoch.so ONLY', 'eb_epoch_last_error',
                  'index_reference', 'adv_stats_reference', 'ppo_log_reference', '4-byte alignment only', 'cycle walking'):
        assert words in text, words


def test_the_existing_tables_and_the_package_surface_are_untouched():
    from env_build_amd import ppo, train
    others = set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES)
    assert not set(epoch.EPOCH_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(epoch.EPOCH_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in epoch.__all__]


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_epoch_sources_are_in_no_list_of_the_other_libraries():
    mine = set(T.UNIT) | {os.path.join('..', '..', 'include', 'envbuild_epoch.h')}
    assert set(eb_build.EPOCH_SOURCES) == {'eb_epoch.hip'} and mine <= set(eb_build.EPOCH_SOURCES + eb_build.EPOCH_HEADERS)
    others = [eb_build.SOURCES, eb_build.HEADERS, eb_build.TRAIN_SOURCES, eb_build.TRAIN_HEADERS] + list(eb_build.KERNEL_SOURCES.values())
    for files in others:
        assert not [f for f in files if 'epoch' in f], files
    # the reverse: no source of another library, and no header that is the training library's alone; the headers shared with the main
    # library are splitmix64's (eb_env_device.h and what it includes), read and never changed
    assert not [f for f in eb_build.EPOCH_SOURCES + eb_build.EPOCH_HEADERS if 'train' in f]
    assert not set(eb_build.EPOCH_SOURCES) & set(eb_build.SOURCES + eb_build.TRAIN_SOURCES)
    shared = set(eb_build.EPOCH_HEADERS) - mine
    assert shared == {'eb_env_device.h', 'eb_device.h', 'eb_kernels.h', os.path.join('..', '..', 'include', 'envbuild.h')} <= set(eb_build.HEADERS)
    assert eb_build.EPOCH_LIB not in (eb_build.LIB, eb_build.TRAIN_LIB) and os.path.dirname(eb_build.EPOCH_LIB) == os.path.dirname(eb_build.LIB)
    assert os.path.basename(eb_build.EPOCH_LIB) == 'libenvbuild_epoch.so'
    assert len({eb_build.epoch_source_hash(), eb_build.train_source_hash(), eb_build.source_hash()}) == 3
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_epoch.hip']
    while todo:
        f = os.path.normpath(todo.pop())
        if f in seen:
            continue
        seen.add(f)
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            for inc in re.findall(r'#include "([^"]+)"', fh.read()):
                todo.append(os.path.join(os.path.dirname(f), inc))
    listed = {os.path.normpath(f) for f in eb_build.EPOCH_SOURCES + eb_build.EPOCH_HEADERS}
    assert seen == listed, (sorted(seen - listed), sorted(listed - seen))
    # no unit of the other libraries includes an epoch header
    for f in eb_build.SOURCES + eb_build.HEADERS + eb_build.TRAIN_SOURCES + eb_build.TRAIN_HEADERS:
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            body = fh.read()
        assert 'eb_epoch' not in body and 'envbuild_epoch' not in body, f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence'):
        assert word not in code, word
    assert '__syncthreads' in code and 'hipMalloc' not in code and 'hipMemcpy' not in code and 'Synchronize' not in code
    assert 'splitmix64' in code and 'eb_env_device.h' in code and '0xBF58476D1CE4E5B9' not in code        # the sampler's, not a copy


def test_the_code_object_holds_exactly_the_five_kernels():
    lib, blob = T.library()
    assert lib.eb_epoch_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 25.'):]
    for k in T.KERNELS:
        assert k in section, k
    # the other two libraries export none of the entries and hold none of the kernels
    for path in (eb_build.build(), eb_build.build_train()):
        other = open(path, 'rb').read()
        for name in list(epoch.EPOCH_PROTOTYPES) + list(T.KERNELS):
            assert name.encode() not in other, (path, name)


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    nan = float('nan')
    assert p % 8 == 0

    def gargs(n_total=16, offset=0, count=4, n_sources=1, width=2, perm=None, perm_bytes=0, counter=None, index_out=None, src=p, dst=p + 128):
        a = epoch.EbGatherArgs(n_total=n_total, offset=offset, count=count, n_sources=n_sources, perm=perm, perm_bytes=perm_bytes,
                               counter=counter, index_out=index_out)
        for k in range(epoch.EB_EPOCH_MAX_SOURCES):
            a.sources[k].src, a.sources[k].dst, a.sources[k].width = src, dst, width
        return C.byref(a)

    def sargs(n=4, x=p, eps=1e-8, out=p, std_out=None, partials=p):
        return C.byref(epoch.EbAdvStatsArgs(n=n, x=x, eps=eps, out=out, std_out=std_out, partials=partials))

    def largs(n=4, clip=0.2, out=p, **kw):
        full = dict(logp=p, logp_old=p, ratio=p, surr=p, ent=p, vloss=p)
        full.update(kw)
        return C.byref(epoch.EbPpoLogArgs(n=n, clip=clip, out=out, **full))

    def vargs(counter=p, by=1):
        return C.byref(epoch.EbEpochAdvanceArgs(counter=counter, by=by))

    calls = [
        ('eb_minibatch_gather', None), ('eb_minibatch_gather', gargs(n_sources=0)), ('eb_minibatch_gather', gargs(n_sources=9)),
        ('eb_minibatch_gather', gargs(width=0)), ('eb_minibatch_gather', gargs(width=4097)), ('eb_minibatch_gather', gargs(perm=p, perm_bytes=3)),
        ('eb_minibatch_gather', gargs(offset=13, count=4)), ('eb_minibatch_gather', gargs(count=-1)), ('eb_minibatch_gather', gargs(offset=-1)),
        ('eb_minibatch_gather', gargs(n_total=2 ** 31, count=4)), ('eb_minibatch_gather', gargs(n_total=2 ** 31, count=2 ** 31)),
        ('eb_minibatch_gather', gargs(src=None)), ('eb_minibatch_gather', gargs(dst=None)), ('eb_minibatch_gather', gargs(src=p + 2)),
        ('eb_minibatch_gather', gargs(dst=p + 1)), ('eb_minibatch_gather', gargs(perm=p + 4, perm_bytes=8)),
        ('eb_minibatch_gather', gargs(perm=p + 2, perm_bytes=4)), ('eb_minibatch_gather', gargs(counter=p + 4)),
        ('eb_minibatch_gather', gargs(index_out=p + 2)),
        ('eb_adv_stats', None), ('eb_adv_stats', sargs(n=1)), ('eb_adv_stats', sargs(n=-1)), ('eb_adv_stats', sargs(n=2 ** 31)),
        ('eb_adv_stats', sargs(eps=nan)), ('eb_adv_stats', sargs(x=None)), ('eb_adv_stats', sargs(out=None)), ('eb_adv_stats', sargs(partials=None)),
        ('eb_adv_stats', sargs(x=p + 2)), ('eb_adv_stats', sargs(out=p + 1)), ('eb_adv_stats', sargs(std_out=p + 2)),
        ('eb_adv_stats', sargs(partials=p + 4)),
        ('eb_ppo_log', None), ('eb_ppo_log', largs(n=-1)), ('eb_ppo_log', largs(n=2 ** 31)), ('eb_ppo_log', largs(clip=nan)),
        ('eb_ppo_log', largs(out=None)), ('eb_ppo_log', largs(out=p + 4)), ('eb_ppo_log', largs(ratio=p + 2)), ('eb_ppo_log', largs(logp=p + 1)),
        ('eb_epoch_advance', None), ('eb_epoch_advance', vargs(counter=None)), ('eb_epoch_advance', vargs(counter=p + 4)),
    ]
    assert len(calls) >= 20
    for name, a in calls:
        assert getattr(lib, name)(a) == -1, name
        assert lib.eb_epoch_last_error().startswith(name.encode() + b':'), (name, lib.eb_epoch_last_error())
    assert all(v == 0.0 for v in buf)
    # a count of 0 is a no-op that needs no pointer and no device
    assert lib.eb_minibatch_gather(gargs(count=0, src=None, dst=None)) == 0
    assert lib.eb_minibatch_gather(gargs(n_total=0, count=0, src=None, dst=None)) == 0
    assert lib.eb_adv_stats(sargs(n=0, x=None, out=None, partials=None)) == 0
    assert lib.eb_ppo_log(largs(n=0, out=None)) == 0
    assert all(v == 0.0 for v in buf)


# ---- 4: the index function is a bijection --------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 1000, 4096, 4097, 65537)


@pytest.mark.parametrize('n', SIZES)
def test_index_reference_is_a_bijection(n):
    for seed, ep, base in ((3, 0, 0), (4, 1, 0), (0, 0, 5)):
        perm, walks = epoch.index_reference(n, seed, ep, base, walks=True)
        assert perm.shape == (n,) and perm.dtype == np.int64
        assert np.array_equal(np.sort(perm), np.arange(n)), (n, seed, ep, base)
        print('n %d, seed %d, epoch %d, base %d: mean walk %.3f, longest %d' % (n, seed, ep, base, walks.mean(), walks.max()))
        assert walks.min() >= 1 and walks.mean() <= 4.0 + 1e-9
        if n == 65537:
            assert walks.max() < 200                                  # a bound that low only catches a broken loop


def test_keys_give_different_permutations_and_base_plus_epoch_is_the_key():
    n = 4096
    first = epoch.index_reference(n, 3, 0)
    for what, other in (('epoch 1', epoch.index_reference(n, 3, 1)), ('seed 4', epoch.index_reference(n, 4, 0)),
                        ('base 1', epoch.index_reference(n, 3, 0, base=1))):
        share = float((first == other).mean())
        print('%s agrees with (seed 3, epoch 0, base 0) in %.4f of the slots' % (what, share))
        assert share < 0.01, what
    assert np.array_equal(epoch.index_reference(n, 3, 0, base=1), epoch.index_reference(n, 3, 1, base=0))
    assert np.array_equal(epoch.index_reference(n, 3, 2, base=5), epoch.index_reference(n, 3, 7))
    assert np.array_equal(first, epoch.index_reference(n, 3, 0))


# ---- 5: coarse uniformity --------------------------------------------------------------------------------------------------------------------
def test_coarse_uniformity_over_512_epochs():
    """n = 4096, one seed, 512 epochs.  Per slot the chi-square of the quarter its source row falls into (4 bins, 3 degrees of freedom):
    mean 3 +- 0.15, at most 1 % of the slots above 16.27 (p = 1e-3); fixed points per epoch 0.8 .. 1.2 on average.
    Measured with 6 rounds: mean 2.982, 0.07 % above 16.27, 0.939 fixed points per epoch."""
    n, epochs = 4096, 512
    perms = np.stack([epoch.index_reference(n, 3, e) for e in range(epochs)])
    quarter = perms // (n // 4)
    expected = epochs / 4.0
    chi = sum((((quarter == b).sum(axis=0) - expected) ** 2) / expected for b in range(4))
    share = float((chi > 16.27).mean())
    fixed = float((perms == np.arange(n)).sum(axis=1).mean())
    print('chi-square per slot: mean %.3f, share above 16.27 %.4f; fixed points per epoch %.3f' % (chi.mean(), share, fixed))
    assert abs(chi.mean() - 3.0) <= 0.15
    assert share <= 0.01
    assert 0.8 <= fixed <= 1.2


# ---- 6: the statistics' restatement ----------------------------------------------------------------------------------------------------------
def stats_data(n, ratio):
    """float32 data N(ratio, 1): mean / std = ratio"""
    rng = np.random.default_rng(1000 * n + int(ratio))
    return (ratio + rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize('ratio', [0, 1, 1000])
@pytest.mark.parametrize('n', [2, 3, 1025, 100003])
def test_adv_stats_reference_against_numpy(n, ratio):
    """float64 restatement against np.mean / np.std(ddof=1) to 1e-12 relative; the float32 one within one float ulp of the rounded float64
    values; inv exactly 1.0f / (std + eps) of its own std.

    The sums are of the deviations from x[0]: with the plain sums of x and x * x the cases at mean / std = 1000 miss this bar (std off by
    3e-12 at n = 3, 2e-12 at 1025 and 4e-11 at 100003, where Q - S^2 / n cancels mean^2 / var = 1e6 of the sums' 2^-53)."""
    x = stats_data(n, ratio)
    x64 = x.astype(np.float64)
    want_mean, want_std = np.mean(x64), np.std(x64, ddof=1)
    mean, inv, std = epoch.adv_stats_reference(x, 1e-8, np.float64)
    print('n %d, mean / std %g: mean off by %.3g relative, std by %.3g' % (n, ratio, abs(mean - want_mean) / max(abs(want_mean), 1e-300),
                                                                            abs(std - want_std) / want_std))
    m32, i32, s32 = epoch.adv_stats_reference(x, 1e-8, np.float32)
    assert all(type(v) is np.float32 for v in (m32, i32, s32))
    assert abs(float(m32) - float(np.float32(want_mean))) <= float(np.spacing(np.float32(abs(want_mean))))
    assert abs(float(s32) - float(np.float32(want_std))) <= float(np.spacing(np.float32(want_std)))
    assert i32 == np.float32(1.0) / (s32 + np.float32(1e-8))
    assert inv == 1.0 / (std + 1e-8)
    assert abs(mean - want_mean) <= 1e-12 * abs(want_mean)
    assert abs(std - want_std) <= 1e-12 * want_std


def test_adv_stats_reference_nan_and_order():
    x = stats_data(1025, 1)
    x[700] = np.nan
    for dtype in (np.float32, np.float64):
        assert all(np.isnan(v) for v in epoch.adv_stats_reference(x, 1e-8, dtype))
    with pytest.raises(ValueError):
        epoch.adv_stats_reference(np.ones(1, np.float32))
    # constant data: the variance is 0 (or clamped to it), std 0 and inv 1 / eps
    mean, inv, std = epoch.adv_stats_reference(np.full(5000, 0.1, np.float32), 1e-8, np.float32)
    assert mean == np.float32(0.1) and std >= 0.0 and std < 1e-6 and np.isfinite(inv)
    # more than 256 chunks: a block takes a second round of chunks
    x = stats_data(300000, 1)
    mean, _, std = epoch.adv_stats_reference(x, 1e-8, np.float64)
    assert abs(mean - np.mean(x.astype(np.float64))) <= 1e-12 and abs(std - np.std(x.astype(np.float64), ddof=1)) <= 1e-12


# ---- 7: the log's restatement ----------------------------------------------------------------------------------------------------------------
def log_inputs(n, seed=0):
    rng = np.random.default_rng(seed + n)
    logp_old = (-1.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    logp = (logp_old + 0.1 * rng.standard_normal(n)).astype(np.float32)
    ratio = np.exp(logp - logp_old).astype(np.float32)
    surr = (ratio * rng.standard_normal(n)).astype(np.float32)
    ent = (1.0 + 0.2 * rng.standard_normal(n)).astype(np.float32)
    vloss = (0.5 * rng.standard_normal(n) ** 2).astype(np.float32)
    return dict(logp=logp, logp_old=logp_old, ratio=ratio, surr=surr, ent=ent, vloss=vloss)


@pytest.mark.parametrize('n', [1, 255, 257, 16385, 40000])
def test_ppo_log_reference_and_fold_against_the_torch_expressions(n):
    """examples/ppo_captured_loop.py's logging expressions on float64 CPU tensors (the clip test and the subtraction in float32, as the
    kernel does them)"""
    import torch
    clip = 0.2
    x = log_inputs(n)
    blocks = epoch.ppo_log_reference(clip=clip, **x)
    assert blocks.shape == (64, 8) and blocks.dtype == np.float64
    got = epoch.fold_log(blocks)
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    want = dict(policy_loss=float(-t['surr'].double().mean()), value_loss=float(t['vloss'].double().mean()), entropy=float(t['ent'].double().mean()),
                approx_kl=float((t['logp_old'] - t['logp']).double().mean()))
    scale = dict(policy_loss=np.abs(x['surr']).sum(dtype=np.float64) / n, value_loss=np.abs(x['vloss']).sum(dtype=np.float64) / n,
                 entropy=np.abs(x['ent']).sum(dtype=np.float64) / n, approx_kl=np.abs(x['logp_old'] - x['logp']).sum(dtype=np.float64) / n)
    for k, w in want.items():
        assert abs(float(got[k]) - w) <= 1e-12 * scale[k], (k, float(got[k]), w)
    assert float(got['clip_fraction']) * n == float(((t['ratio'] - 1.0).abs() > clip).sum())
    assert float(got['clip_fraction']) == float(((t['ratio'] - 1.0).abs() > clip).double().mean())
    assert float(got['max_ratio_dev']) == float((t['ratio'] - 1.0).abs().max())
    assert float(got['nonfinite_rows']) == 0.0 and float(got['rows']) == n
    # the blocks' row counts are the kernel's cut: block b holds the rows b * 256 + t + k * 16384
    rows = np.arange(n)
    assert np.array_equal(blocks[:, 7], np.bincount((rows % 16384) // 256, minlength=64))


def test_ppo_log_reference_missing_inputs_and_bad_rows():
    n = 600
    x = log_inputs(n)
    full = epoch.ppo_log_reference(clip=0.2, **x)
    for gone in x:
        part = epoch.ppo_log_reference(clip=0.2, **{k: (None if k == gone else v) for k, v in x.items()})
        zero = {'surr': [0], 'vloss': [1], 'ent': [2], 'ratio': [3, 5], 'logp': [4], 'logp_old': [4]}[gone]
        for f in range(8):
            assert (part[:, f] == 0.0).all() if f in zero else np.array_equal(part[:, f], full[:, f]), (gone, f)
    x['ratio'][5], x['surr'][300], x['logp'][300], x['ent'][599] = np.nan, np.inf, -np.inf, np.nan
    bad = epoch.ppo_log_reference(clip=0.2, **x)
    assert bad[:, 6].sum() == 3 and bad[0, 6] == 1 and bad[1, 6] == 1 and bad[2, 6] == 1
    assert np.isfinite(bad[:, 5]).all() and bad[:, 5].max() == np.nanmax(np.abs(x['ratio'] - np.float32(1.0)))
    folded = epoch.fold_log(np.stack([full, bad]))
    assert folded['rows'].shape == (2,) and folded['nonfinite_rows'].tolist() == [0.0, 3.0]
    with pytest.raises(ValueError):
        epoch.fold_log(np.zeros((3, 8)))
