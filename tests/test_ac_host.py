"""CPU (-m "not gpu"): the shared-trunk actor-critic family (include/envbuild_ac.h, env_build_amd.ac) — its header against the module's
binding table and argument structs, the separation of libenvbuild_ac.so from the other five libraries and the kernels its code object
holds, device-free refusals, and the two NumPy restatements against the compositions they are made of, on strided arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import ac, collect, ctl, epoch, ppo, train
from env_build_amd import policy_sample as ps
from tests import _ac as T
from tests import _kernel_census as K
from tests._helpers import ROOT

STRUCTS = {'eb_ac_loss_args': ac.EbAcLossArgs, 'eb_ac_sample_args': ac.EbAcSampleArgs}
PROTOTYPES = {                                                     # include/envbuild_ac.h, written out: (result, parameters)
    'eb_ac_abi_version': ('int', 'void'),
    'eb_ac_last_error': ('const char*', 'void'),
    'eb_ac_loss': ('int', 'const eb_ac_loss_args*'),
    'eb_ac_sample': ('int', 'const eb_ac_sample_args*'),
}
LOSS_FIELDS = [('n', C.c_int32), ('act_dim', C.c_int32)] + [(k, C.c_void_p) for k in ('y', 'actions', 'logp_old', 'adv', 'adv_norm', 'ret', 'v_old')] \
    + [(k, C.c_float) for k in ('action_range', 'clip', 'ent_coef', 'scale', 'clip_v', 'v_scale')] \
    + [(k, C.c_void_p) for k in ('logp', 'ratio', 'surr', 'ent', 'vloss', 'g_y', 'z_out', 'stream')]
SAMPLE_FIELDS = [('n', C.c_int32), ('act_dim', C.c_int32), ('y', C.c_void_p), ('eps', C.c_void_p), ('row_ids', C.c_void_p), ('seed', C.c_uint64),
                 ('counter', C.c_uint64), ('action_range', C.c_float)] \
    + [(k, C.c_void_p) for k in ('actions', 'logits_out', 'values', 'logp', 'eps_out', 'stream')]


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_against_the_prototype_table():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(PROTOTYPES) == sorted(ac.AC_PROTOTYPES) == sorted(T.ENTRIES + ('eb_ac_abi_version', 'eb_ac_last_error'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in STRUCTS.items()}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, params) in PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and m.group(1) == res and ' '.join(m.group(2).split()) == params, name
        bound_res, bound_args = ac.AC_PROTOTYPES[name]
        assert results[res] is bound_res, name
        assert [kinds[p] for p in [params] if p != 'void'] == bound_args, name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    macros = {m: getattr(ac, m) for m in ('EB_AC_ABI_VERSION', 'EB_AC_MAX_ACT_DIM')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_AC_\w+) ', text)) == sorted(macros) and tuple(macros.values()) == (1, 15)
    for words in ('bit for bit', 'AT CALL TIME', 'tests/test_stream_census.py', 'ALWAYS exactly ONE launch', 'libenvbuild_ac.so ONLY',
                  'eb_ac_last_error', 'ac_loss_reference', 'ac_sample_reference', 'restates NO arithmetic', 'SPLIT ONLY', 'W is odd',
                  'Every column of g_y is written'):
        assert words in text, words


def test_the_capture_test_holds_both_entries_as_the_struct_census_asks():
    """tests/_capture_cases.py's table of struct-taking entries (STRUCT_STREAM_HELD) is a fixed list of the other families' twenty; the
    header declares these two prototypes without a parameter name, which that parser passes over.  The obligation itself is applied here,
    with the census's own function_text: the named GPU test mentions the entry, runs it on a side stream, captures and replays it."""
    from tests._capture_cases import STRUCT_STREAM_HELD, function_text, struct_stream_entries
    _, src = T.header()
    for entry, struct in (('eb_ac_loss', 'eb_ac_loss_args'), ('eb_ac_sample', 'eb_ac_sample_args')):
        assert re.search(r'\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*\)\s*;' % (entry, struct), src), entry
        assert ('stream', C.c_void_p) in T.struct_fields(src, struct)
        assert entry not in STRUCT_STREAM_HELD and entry not in struct_stream_entries()
        text = function_text('test_gpu_ac', 'test_both_entries_on_a_side_stream_and_under_capture')
        assert text is not None and re.search(r"['\"]%s['\"]" % entry, text), entry
        assert 'side' in text and re.search(r'\bcapture\(', text) and 'replay' in text, entry


def test_the_structs_in_field_order_and_types():
    _, src = T.header()
    assert T.struct_fields(src, 'eb_ac_loss_args') == list(ac.EbAcLossArgs._fields_) == LOSS_FIELDS
    assert T.struct_fields(src, 'eb_ac_sample_args') == list(ac.EbAcSampleArgs._fields_) == SAMPLE_FIELDS
    for struct in STRUCTS.values():
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    assert ac.EbAcLossArgs.y.offset == 8 and ac.EbAcSampleArgs.seed.offset == 32 and ac.EbAcSampleArgs.actions.offset == 56


def test_the_existing_tables_and_the_package_surface_are_untouched():
    others = (set(_capi.PROTOTYPES) | set(ppo.PPO_PROTOTYPES) | set(train.TRAIN_PROTOTYPES) | set(epoch.EPOCH_PROTOTYPES)
              | set(collect.COLLECT_PROTOTYPES) | set(ctl.CTL_PROTOTYPES))
    assert not set(ac.AC_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(ac.AC_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in ac.__all__]
    assert issubclass(ac.PPOUpdate, train.PPOUpdate) and not issubclass(ac.PPOUpdate, ctl.PPOUpdate)
    assert issubclass(ac.ControlledPPOUpdate, ac.PPOUpdate) and issubclass(ac.ControlledPPOUpdate, ctl.PPOUpdate)
    assert ac.ControlledPPOUpdate.step is ac.PPOUpdate.step and ac.ControlledPPOUpdate._make_adam is ac.PPOUpdate._make_adam
    assert ac.PPOUpdate.capture is train.PPOUpdate.capture and ac.PPOUpdate.replay is train.PPOUpdate.replay
    assert issubclass(ac.Collector, collect.Collector) and ac.Collector.episodes is collect.Collector.episodes


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_ac_sources_are_in_no_list_of_the_other_libraries():
    inc = lambda f: os.path.join('..', '..', 'include', f)
    mine = set(T.UNIT) | {inc('envbuild_ac.h')}
    own = eb_build.AC_SOURCES + eb_build.AC_HEADERS
    assert eb_build.AC_SOURCES == ['eb_ac.hip'] and mine <= set(own) and len(own) == len(set(own))
    others = [eb_build.SOURCES, eb_build.HEADERS, eb_build.TRAIN_SOURCES, eb_build.TRAIN_HEADERS, eb_build.EPOCH_SOURCES,
              eb_build.EPOCH_HEADERS, eb_build.COLLECT_SOURCES, eb_build.COLLECT_HEADERS, eb_build.CTL_SOURCES, eb_build.CTL_HEADERS]
    for files in others + list(eb_build.KERNEL_SOURCES.values()):
        assert not mine & set(files), files
    # what it borrows: device headers of the main and the train library, listed there too, unchanged
    assert set(own) - mine <= set(eb_build.HEADERS) | set(eb_build.TRAIN_HEADERS)
    libs = (eb_build.LIB, eb_build.TRAIN_LIB, eb_build.EPOCH_LIB, eb_build.COLLECT_LIB, eb_build.CTL_LIB)
    assert eb_build.AC_LIB not in libs
    assert os.path.dirname(eb_build.AC_LIB) == os.path.dirname(eb_build.LIB) and os.path.basename(eb_build.AC_LIB) == 'libenvbuild_ac.so'
    assert len({eb_build.ac_source_hash(), eb_build.ctl_source_hash(), eb_build.collect_source_hash(), eb_build.epoch_source_hash(),
                eb_build.train_source_hash(), eb_build.source_hash()}) == 6
    # every file the unit includes, transitively, is in the library's lists, and nothing else is
    seen, todo = set(), ['eb_ac.hip']
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
    # no unit of the other libraries includes an ac header
    for f in set(sum(others, [])):
        with open(os.path.join(eb_build.CSRC, f)) as fh:
            body = fh.read()
        assert not re.search(r'\beb_ac[._]|\benvbuild_ac\b|\bac_(loss|sample)_kernel\b', body), f
    # the unit calls the row functions and writes none of them; it makes two launches and nothing that allocates, copies or waits
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for call in ('plogp::logp_row(', 'plogp::logp_vjp_elem(', 'mlp::exp_det(', 'train::value_loss_row(', 'psample::sample_row('):
        assert code.count(call) == 1, call
    for word in ('hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize', '__syncthreads', '__shfl', 'fmaf', 'expf', 'logf', 'tanhf'):
        assert word not in code, word
    assert code.count('hipLaunchKernelGGL') == 2 and set(re.findall(r'__global__[^\n]*void (\w+)\(', code)) == set(T.KERNELS)
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert entry.count('_b.build_ac()') == 1


def test_the_code_object_holds_exactly_the_two_kernels():
    lib, blob = T.library()
    assert lib.eb_ac_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 28.'):]
    for k in T.KERNELS:
        assert k in section, k
    # the other five libraries export none of the entries and hold none of the kernels
    for path in (eb_build.build(), eb_build.build_train(), eb_build.build_epoch(), eb_build.build_collect(), eb_build.build_ctl()):
        other = open(path, 'rb').read()
        for name in list(ac.AC_PROTOTYPES) + list(T.KERNELS):
            assert name.encode() not in other, (path, name)


# ---- 3: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert p % 4 == 0
    nan = float('nan')

    def largs(**kw):
        full = dict(n=4, act_dim=2, action_range=1.0, clip=0.2, ent_coef=1e-3, scale=0.25, clip_v=0.2, v_scale=0.125)
        full.update({k: p for k in ('y', 'actions', 'logp_old', 'adv', 'adv_norm', 'ret', 'v_old', 'logp', 'ratio', 'surr', 'ent', 'vloss', 'g_y', 'z_out')})
        full.update(kw)
        return C.byref(ac.EbAcLossArgs(**full))

    def sargs(**kw):
        full = dict(n=4, act_dim=2, seed=1, counter=2, action_range=1.0)
        full.update({k: p for k in ('y', 'eps', 'row_ids', 'actions', 'logits_out', 'values', 'logp', 'eps_out')})
        full.update(kw)
        return C.byref(ac.EbAcSampleArgs(**full))

    calls = [('eb_ac_loss', None), ('eb_ac_loss', largs(n=-1)), ('eb_ac_loss', largs(act_dim=0)), ('eb_ac_loss', largs(act_dim=16)),
             ('eb_ac_loss', largs(act_dim=-1)), ('eb_ac_loss', largs(clip=-0.1)), ('eb_ac_loss', largs(clip_v=-0.1)), ('eb_ac_loss', largs(clip_v=nan))]
    calls += [('eb_ac_loss', largs(**{k: nan})) for k in ('action_range', 'clip', 'ent_coef', 'scale', 'v_scale')]
    calls += [('eb_ac_loss', largs(**{k: None})) for k in ('y', 'actions', 'logp_old', 'adv', 'ret', 'logp')]
    calls += [('eb_ac_loss', largs(**{k: p + 2})) for k in ('y', 'actions', 'logp_old', 'adv', 'adv_norm', 'ret', 'v_old', 'logp', 'ratio', 'surr',
                                                             'ent', 'vloss', 'g_y', 'z_out')]
    calls += [('eb_ac_loss', largs(n=0, act_dim=16)), ('eb_ac_loss', largs(n=0, scale=nan))]
    calls += [('eb_ac_sample', None), ('eb_ac_sample', sargs(n=-1)), ('eb_ac_sample', sargs(act_dim=0)), ('eb_ac_sample', sargs(act_dim=16)),
              ('eb_ac_sample', sargs(action_range=nan)), ('eb_ac_sample', sargs(y=None)),
              ('eb_ac_sample', sargs(actions=None, logits_out=None, values=None)), ('eb_ac_sample', sargs(n=0, act_dim=0))]
    calls += [('eb_ac_sample', sargs(**{k: p + 1})) for k in ('y', 'eps', 'row_ids', 'actions', 'logits_out', 'values', 'logp', 'eps_out')]
    assert len(calls) >= 50 and {name for name, _ in calls} == set(T.ENTRIES)
    for k, (name, a) in enumerate(calls):
        assert getattr(lib, name)(a) == -1, (name, k)
        assert lib.eb_ac_last_error().startswith(name.encode() + b':'), (name, lib.eb_ac_last_error())
    assert all(v == 0.0 for v in buf)
    # no rows: no-ops that need no pointer and no device
    none = {k: None for k in ('y', 'actions', 'logp_old', 'adv', 'adv_norm', 'ret', 'v_old', 'logp', 'ratio', 'surr', 'ent', 'vloss', 'g_y', 'z_out')}
    assert lib.eb_ac_loss(largs(n=0, **none)) == 0
    assert lib.eb_ac_loss(largs(n=0, clip_v=nan, v_old=None)) == 0            # clip_v is not read without v_old
    assert lib.eb_ac_sample(sargs(n=0, **{k: None for k in ('y', 'eps', 'row_ids', 'actions', 'logits_out', 'values', 'logp', 'eps_out')})) == 0
    assert all(v == 0.0 for v in buf)


def test_the_python_surface_refuses_what_it_cannot_run():
    for bad in (0, 16, -1):
        with pytest.raises(ValueError):
            ac.make_net(41, 2, 64, 'elu', bad)
    with pytest.raises(ValueError):
        ac.make_net(41, 2, 64, 'elu', 2, output_activation='tanh')
    for out_dim in (2, 4, 1, 33):
        with pytest.raises(ValueError):
            ac._act_dim(out_dim)
    assert [ac._act_dim(w) for w in (3, 5, 31)] == [1, 2, 15]
    with pytest.raises(TypeError):
        ac.split(object())
    with pytest.raises(ValueError):
        ac.ac_loss_reference(np.zeros((3, 4), np.float32), np.zeros((3, 2)), np.zeros(3), np.zeros(3), np.zeros(3), 1.0, 0.2)
    with pytest.raises(ValueError):
        ac.ac_sample_reference(np.zeros(5, np.float32), np.zeros((1, 2)), 1.0)


# ---- 4: the restatements are their compositions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('action_range', T.RANGES)
@pytest.mark.parametrize('act_dim', T.ACT_DIMS)
def test_ac_loss_reference_is_the_composition_on_strided_arrays(act_dim, action_range):
    n = 65
    case = T.loss_case(n, act_dim, action_range)
    y = case['y']
    A2 = 2 * act_dim
    assert not y[:, :A2].flags['C_CONTIGUOUS'] and y[:, A2].strides == (4 * (A2 + 1),)
    for clip in (T.CLIP, 0.0):
        for with_norm in (True, False):
            for with_v_old in (True, False):
                got = T.loss_reference(case, action_range, clip, with_norm, with_v_old)
                want = ppo.ppo_reference(np.ascontiguousarray(y[:, :A2]), case['actions'], case['logp_old'], case['adv'], action_range, clip,
                                         ent_coef=T.ENT_COEF, scale=1.0 / n, adv_norm=T.ADV_NORM if with_norm else None)
                vloss, g_v = train.value_loss_reference(np.ascontiguousarray(y[:, A2]), case['ret'], case['v_old'] if with_v_old else None,
                                                        clip_v=T.CLIP_V, scale=T.VF_COEF / n)
                for k in ('logp', 'z', 'A', 'ratio', 'surr', 'ent', 'g_lp'):
                    assert T.same(got[k], want[k]), k
                assert T.same(got['vloss'], vloss) and T.same(got['g_y'][:, :A2], want['g_logits']) and T.same(got['g_y'][:, A2], g_v)
                assert got['g_y'].shape == (n, A2 + 1) and got['g_y'].dtype == np.float32
                assert not T.every_branch_is_taken(case, got, clip, with_v_old), T.every_branch_is_taken(case, got, clip, with_v_old)
                # a planted NaN poisons its own row only: the logit's the policy columns, the value's the value column, logp_old's the ratio
                bad_policy = np.isnan(got['g_y'][:, :A2]).any(axis=1) | np.isnan(got['logp']) | np.isnan(got['ratio']) | np.isnan(got['surr'])
                assert sorted(np.flatnonzero(bad_policy)) == [T.NAN_LOGIT_ROW, T.NAN_OLD_ROW]
                assert np.isnan(got['logp'][T.NAN_LOGIT_ROW]) and not np.isnan(got['logp'][T.NAN_OLD_ROW])
                bad_value = np.isnan(got['g_y'][:, A2]) | np.isnan(got['vloss'])
                assert list(np.flatnonzero(bad_value)) == [T.NAN_VALUE_ROW]
    f64 = ac.ac_loss_reference(y, case['actions'], case['logp_old'], case['adv'], case['ret'], action_range, T.CLIP, v_old=case['v_old'], clip_v=T.CLIP_V,
                               dtype=np.float64)
    assert f64['g_y'].dtype == np.float64 and f64['g_y'].shape == (n, A2 + 1)


@pytest.mark.parametrize('action_range', T.RANGES)
@pytest.mark.parametrize('act_dim', T.ACT_DIMS)
def test_ac_sample_reference_is_the_composition_on_strided_arrays(act_dim, action_range):
    n = 65
    case = T.loss_case(n, act_dim, action_range)
    y, A2 = case['y'], 2 * act_dim
    eps = ps.policy_noise_reference(np.arange(n), act_dim, 7, 3)
    got = ac.ac_sample_reference(y, eps, action_range)
    actions, logp, _ = ps.policy_sample_reference(np.ascontiguousarray(y[:, :A2]), eps, action_range)
    assert T.same(got['actions'], actions) and T.same(got['logp'], logp)
    assert T.same(got['logits'], y[:, :A2]) and T.same(got['values'], y[:, A2]) and got['logits'].flags['C_CONTIGUOUS']
    bad = np.isnan(got['actions']).any(axis=1) | np.isnan(got['logp'])
    assert list(np.flatnonzero(bad)) == [T.NAN_LOGIT_ROW]                    # the value column's NaN reaches no action
    assert list(np.flatnonzero(np.isnan(got['values']))) == [T.NAN_VALUE_ROW]
