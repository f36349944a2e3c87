"""CPU (-m "not gpu"): the off-policy family (include/envbuild_offpolicy.h, env_build_amd.offpolicy) — its header against the module's
binding table and argument structs, the separation of libenvbuild_offpolicy.so from the other seven libraries and the kernels its code
object holds, device-free refusals and no-ops, and the NumPy restatements: ring slots across the wrap and the next_obs / nonterminal rule
against plain loops, the keyed index's range, keys and coarse uniformity, the critic and actor rows against a float64 evaluation of the same
formulas under the derived bars, and the Polyak step against a scalar loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import offpolicy as O
from env_build_amd.policy_sample import _libm
from tests import _kernel_census as K
from tests import _offpolicy as T
from tests._helpers import ROOT

OTHERS = ('', 'train_', 'epoch_', 'collect_', 'ctl_', 'ac_', 'norm_')


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def test_header_declares_what_the_module_binds():
    text, src = T.header()
    names = sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(O.OFFPOLICY_PROTOTYPES) == sorted(T.ENTRIES + ('eb_offpolicy_abi_version', 'eb_offpolicy_last_error'))
    kinds = {'const %s*' % name: C.POINTER(struct) for name, struct in T.STRUCTS.items()}
    results = {'int': C.c_int, 'const char*': C.c_char_p}
    for name, (res, args) in O.OFFPOLICY_PROTOTYPES.items():
        m = re.search(r'(\bint|\bconst char\*)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and results[m.group(1)] is res, name
        params = [a.strip() for a in m.group(2).split(',') if a.strip() != 'void']
        assert [kinds[p] for p in params] == args, name                       # no parameter name: the type is the whole parameter
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\beb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)             # the stream is a field of the struct
    macros = {m: getattr(O, m) for m in ('EB_OFFPOLICY_ABI_VERSION', 'EB_OFFPOLICY_MAX_OBS', 'EB_OFFPOLICY_MAX_ACT', 'EB_OFFPOLICY_ROWS',
                                         'EB_OFFPOLICY_ALPHA_BLOCKS', 'EB_OFFPOLICY_MAX_SEGMENTS')}
    for macro, value in macros.items():
        assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value, macro
    assert sorted(re.findall(r'#define (EB_OFFPOLICY_\w+) ', text)) == sorted(macros) and tuple(macros.values()) == (1, 4096, 16, 32, 64, 32)
    for name, struct in T.STRUCTS.items():
        assert T.fields_of(src, name) == list(struct._fields_), name
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    assert T.fields_of(src, 'eb_polyak_segment') == list(O.EbPolyakSegment._fields_)
    for words in ('libenvbuild_offpolicy.so ONLY', 'eb_offpolicy_last_error', 'AT CALL TIME', 'tests/test_stream_census.py', 'exactly TWO',
                  'ONE launch', 'a NaN in either travels', '0x7FC00000', 'mulhi64', 'never in memory', 'eb_epoch_advance', 'time-limit truncation',
                  'never in the reset row', 'not read *fill', 'No atomics, no last-block ticket', 'fmaf(tau, o - t, t)', 'push_reference',
                  'sample_index_reference', 'actor_reference', 'polyak_reference', 'noise_id_out', 'read by the kernel'):
        assert words in text, words


def test_the_capture_test_holds_every_entry_as_the_struct_census_asks():
    """tests/_capture_cases.py's tables are fixed lists of the other families' entries; the header declares these seven prototypes without a
    parameter name, which that parser passes over.  The obligation itself is applied here, with the census's own function_text: the named
    GPU test mentions the entry, runs it on a side stream, captures and replays it."""
    from tests._capture_cases import STRUCT_STREAM_HELD, function_text, stream_entries, struct_stream_entries
    _, src = T.header()
    text = function_text('test_gpu_offpolicy', 'test_every_entry_on_a_side_stream_and_under_capture')
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
              | set(collect.COLLECT_PROTOTYPES) | set(ctl.CTL_PROTOTYPES) | set(ac.AC_PROTOTYPES) | set(norm.NORM_PROTOTYPES))
    assert not set(O.OFFPOLICY_PROTOTYPES) & others
    for row in _capi.FAMILIES.values():
        assert not set(O.OFFPOLICY_PROTOTYPES) & set(row[5])
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in O.__all__]


# ---- 2: a library of its own ---------------------------------------------------------------------------------------------------------------
def test_the_offpolicy_sources_are_in_no_list_of_the_other_libraries():
    header = os.path.join('..', '..', 'include', 'envbuild_offpolicy.h')
    mine = set(T.UNIT) | {header}
    own = eb_build.OFFPOLICY_SOURCES + eb_build.OFFPOLICY_HEADERS
    assert eb_build.OFFPOLICY_SOURCES == ['eb_offpolicy.hip'] and mine <= set(own)
    lists = [getattr(eb_build, (p.upper() + kind)) for p in OTHERS for kind in ('SOURCES', 'HEADERS')]
    for files in lists + list(eb_build.KERNEL_SOURCES.values()):
        assert not [f for f in files if 'offpolicy' in f], files
    # what it borrows is read and never changed: exp_det's and splitmix64's headers with what they include, and the return codes' header
    assert set(own) - mine == {'eb_mlp_device.h', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h', os.path.join('..', '..', 'include', 'envbuild.h')}
    assert set(own) - mine <= set(eb_build.HEADERS)
    libs = [getattr(eb_build, p.upper() + 'LIB') for p in OTHERS]
    assert eb_build.OFFPOLICY_LIB not in libs and os.path.dirname(eb_build.OFFPOLICY_LIB) == os.path.dirname(eb_build.LIB)
    assert os.path.basename(eb_build.OFFPOLICY_LIB) == 'libenvbuild_offpolicy.so'
    hashes = {getattr(eb_build, p + 'source_hash')() for p in OTHERS} | {eb_build.offpolicy_source_hash()}
    assert len(hashes) == 8
    # every file the unit includes, transitively, is in the library's lists
    seen, todo = set(), ['eb_offpolicy.hip']
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
    # no unit of the other libraries includes an off-policy header
    for files in lists:
        for f in files:
            with open(os.path.join(eb_build.CSRC, f)) as fh:
                body = fh.read()
            assert 'eb_offpolicy' not in body and 'envbuild_offpolicy' not in body, f
    # kernel code rules: plain C++, __syncthreads only, no atomics, no inline assembly, nothing allocates, copies or synchronises
    unit = ''.join(open(os.path.join(eb_build.CSRC, f)).read() for f in T.UNIT)
    code = re.sub(r'//[^\n]*|/\*.*?\*/', '', unit, flags=re.S)
    for word in ('atomic', 'asm', '__builtin_amdgcn', '__shfl', '__threadfence', 'hipMalloc', 'hipMemcpy', 'hipMemset', 'Synchronize'):
        assert word not in code, word
    assert '__syncthreads' in code and 'float4' in code and 'long long' in code and code.count('__builtin_fmaf') == 2
    assert '-ffp-contract=off' in eb_build.FLAGS
    # the build entry compiles it; the smoke run is as it was
    entry = open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert '_b.build_offpolicy()' in entry and 'offpolicy' not in entry[entry.index('def smoke'):]


def test_the_code_object_holds_exactly_the_eight_kernels():
    lib, blob = T.library()
    assert lib.eb_offpolicy_abi_version() == 1
    kernels = [K.parse(s) for s in K.kernel_symbols(blob)]
    assert sorted(k.family for k in kernels) == sorted(T.KERNELS), [k.symbol for k in kernels]
    assert all(k.args == () for k in kernels)
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 30.'):]
    for k in T.KERNELS:
        assert k in section, k
    assert re.search(r'%d kernel' % O.SAC.KERNELS, section)


# ---- 3: refusals and no-ops ------------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device_and_name_their_entry():
    lib, _ = T.library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert p % 8 == 0
    big, nan = 2 ** 31 - 1, float('nan')
    pointers = {
        'eb_replay_push': ('obs', 'act', 'rew', 'next_obs', 'nonterminal', 'fill', 'prev_obs', 'action', 'reward', 'obs_after', 'done_code', 'final_obs'),
        'eb_replay_sample': ('obs', 'act', 'rew', 'next_obs', 'nonterminal', 'fill', 'counter', 'indices', 'obs_out', 'qin_out', 'next_obs_out',
                             'rew_out', 'nonterminal_out', 'index_out', 'noise_id_out'),
        'eb_q_pack': ('obs', 'act', 'qin'),
        'eb_sac_critic': ('q1t', 'q2t', 'logp_next', 'rew', 'nonterminal', 'q1', 'q2', 'log_alpha', 'y', 'loss1', 'loss2', 'g_q1', 'g_q2'),
        'eb_sac_actor': ('q1', 'q2', 'logp', 'log_alpha', 'loss', 'g_q1', 'g_q2', 'g_logp', 'g_log_alpha', 'partials'),
        'eb_q_action_grad': ('g_in1', 'g_in2', 'g_a'),
    }
    scalars = {
        'eb_replay_push': dict(capacity=8, n=4, start=6, obs_dim=3, act_dim=2, fill_after=4),
        'eb_replay_sample': dict(capacity=8, m=4, obs_dim=3, act_dim=2, seed=1, draw=2, index_bytes=4),
        'eb_q_pack': dict(m=4, obs_dim=3, act_dim=2),
        'eb_sac_critic': dict(m=4, alpha=0.2, gamma=0.99, reward_scale=1.0, inv_m=0.25),
        'eb_sac_actor': dict(m=4, alpha=0.2, inv_m=0.25, target_entropy=-2.0),
        'eb_q_action_grad': dict(m=4, obs_dim=3, act_dim=2),
    }

    def args(entry, **kw):
        full = dict(scalars[entry], **{k: p for k in pointers[entry]})
        full.update(kw)
        return C.byref(T.STRUCTS[T.STRUCT_OF[entry]](**full))

    def polyak(n=2, tau=0.005, **seg):
        a = O.EbPolyakArgs(n_segments=n, tau=tau)
        for k in range(max(0, min(n, 32))):
            s = dict(dict(target=p, online=p + 64, count=4), **seg)
            a.segments[k].target, a.segments[k].online, a.segments[k].count = s['target'], s['online'], s['count']
        return C.byref(a)

    P, Sm, Q, Cr, Ac, G, Y = T.ENTRIES
    calls = [(e, None) for e in T.ENTRIES]
    calls += [(P, args(P, capacity=0)), (P, args(P, n=-1)), (P, args(P, n=9)), (P, args(P, start=-1)), (P, args(P, start=8)),
              (P, args(P, obs_dim=0)), (P, args(P, obs_dim=4097)), (P, args(P, act_dim=0)), (P, args(P, act_dim=17)),
              (P, args(P, capacity=big, n=1, start=0, obs_dim=2)), (P, args(P, prev_obs=None, action=None, reward=None, obs_after=None, done_code=None, final_obs=None)),
              (P, args(P, prev_obs=None)), (P, args(P, action=None)), (P, args(P, reward=None)), (P, args(P, obs_after=None)), (P, args(P, done_code=None)),
              (P, args(P, reward=None, obs_after=None, done_code=None)), (P, args(P, fill_after=-1)), (P, args(P, fill_after=9)), (P, args(P, fill=p + 4))]
    calls += [(P, args(P, **{k: v})) for k in ('obs', 'act', 'rew', 'next_obs', 'nonterminal', 'fill') for v in (None, p + 2)]
    calls += [(P, args(P, **{k: p + 2})) for k in ('prev_obs', 'action', 'reward', 'obs_after', 'final_obs')]
    calls += [(Sm, args(Sm, capacity=0)), (Sm, args(Sm, m=-1)), (Sm, args(Sm, obs_dim=0)), (Sm, args(Sm, act_dim=17)), (Sm, args(Sm, m=big, obs_dim=1, act_dim=1)),
              (Sm, args(Sm, **{k + '_out': None for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal', 'index', 'noise_id')})),
              (Sm, args(Sm, fill=None)), (Sm, args(Sm, fill=p + 4)), (Sm, args(Sm, counter=p + 4)), (Sm, args(Sm, index_bytes=2)),
              (Sm, args(Sm, index_bytes=8, indices=p + 4))]
    calls += [(Sm, args(Sm, **{k: v})) for k in ('obs', 'act', 'rew', 'next_obs', 'nonterminal') for v in (None, p + 2)]
    calls += [(Sm, args(Sm, **{k: p + 2})) for k in ('obs_out', 'qin_out', 'next_obs_out', 'rew_out', 'nonterminal_out', 'index_out', 'noise_id_out')]
    calls += [(Q, args(Q, m=-1)), (Q, args(Q, obs_dim=4097)), (Q, args(Q, act_dim=0)), (Q, args(Q, m=big, obs_dim=1, act_dim=1)), (Q, args(Q, obs=None, act=None)),
              (Q, args(Q, qin=None)), (Q, args(Q, qin=p + 2)), (Q, args(Q, obs=p + 2)), (Q, args(Q, act=p + 2))]
    calls += [(Cr, args(Cr, m=-1)), (Cr, args(Cr, gamma=nan)), (Cr, args(Cr, reward_scale=nan)), (Cr, args(Cr, inv_m=nan)), (Cr, args(Cr, alpha=nan, log_alpha=None)),
              (Cr, args(Cr, y=None, loss1=None, loss2=None, g_q1=None, g_q2=None)), (Cr, args(Cr, q1=None)), (Cr, args(Cr, q2=None)), (Cr, args(Cr, log_alpha=p + 2))]
    calls += [(Cr, args(Cr, **{k: v})) for k in ('q1t', 'q2t', 'logp_next', 'rew', 'nonterminal') for v in (None, p + 2)]
    calls += [(Cr, args(Cr, **{k: p + 2})) for k in ('y', 'loss1', 'loss2', 'g_q1', 'g_q2', 'q1', 'q2')]
    calls += [(Ac, args(Ac, m=-1)), (Ac, args(Ac, inv_m=nan)), (Ac, args(Ac, alpha=nan, log_alpha=None)), (Ac, args(Ac, target_entropy=nan)),
              (Ac, args(Ac, loss=None, g_q1=None, g_q2=None, g_logp=None, g_log_alpha=None)), (Ac, args(Ac, partials=None)), (Ac, args(Ac, partials=p + 4))]
    calls += [(Ac, args(Ac, **{k: v})) for k in ('q1', 'q2', 'logp') for v in (None, p + 2)]
    calls += [(Ac, args(Ac, **{k: p + 2})) for k in ('log_alpha', 'loss', 'g_q1', 'g_q2', 'g_logp', 'g_log_alpha')]
    calls += [(G, args(G, m=-1)), (G, args(G, obs_dim=0)), (G, args(G, act_dim=17)), (G, args(G, m=big, obs_dim=1, act_dim=1)), (G, args(G, g_in1=None)),
              (G, args(G, g_a=None)), (G, args(G, g_in1=p + 2)), (G, args(G, g_in2=p + 2)), (G, args(G, g_a=p + 2))]
    calls += [(Y, polyak(n=-1)), (Y, polyak(n=33)), (Y, polyak(tau=nan)), (Y, polyak(count=-1)), (Y, polyak(count=2 ** 31)), (Y, polyak(count=2 ** 30 + 1)),
              (Y, polyak(target=None)), (Y, polyak(online=None)), (Y, polyak(target=p + 2)), (Y, polyak(online=p + 2)), (Y, polyak(online=p))]
    assert len(calls) >= 120 and {name for name, _ in calls} == set(T.ENTRIES)
    for k, (name, a) in enumerate(calls):
        assert getattr(lib, name)(a) == -1, (k, name)
        assert lib.eb_offpolicy_last_error().startswith(name.encode() + b':'), (name, lib.eb_offpolicy_last_error())
    assert all(v == 0.0 for v in buf)
    # a NaN target_entropy is read only with g_log_alpha; no rows, no segments, no elements: no-ops that need no pointer and no device
    none = lambda e: {k: None for k in pointers[e]}
    assert lib.eb_replay_push(args(P, n=0, **none(P))) == 0 and lib.eb_replay_sample(args(Sm, m=0, **none(Sm))) == 0
    assert lib.eb_q_pack(args(Q, m=0, **none(Q))) == 0 and lib.eb_sac_critic(args(Cr, m=0, **none(Cr))) == 0
    assert lib.eb_sac_actor(args(Ac, m=0, target_entropy=nan, **none(Ac))) == 0 and lib.eb_q_action_grad(args(G, m=0, **none(G))) == 0
    assert lib.eb_polyak(polyak(n=0)) == 0 and lib.eb_polyak(polyak(n=32, count=0, target=None, online=None)) == 0
    assert all(v == 0.0 for v in buf)
    # the module's own refusals
    with pytest.raises(ValueError):
        O._dims(0, 2)
    with pytest.raises(ValueError):
        O._dims(41, 17)


# ---- 4: the ring's restatements against plain loops ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('final', [False, True])
@pytest.mark.parametrize('C_,n,start', [(5, 3, 4), (5, 5, 2), (64, 64, 63), (257, 65, 192), (257, 65, 256), (257, 1, 256), (7, 3, 0)])
def test_push_reference_against_a_plain_loop(C_, n, start, final):
    D, A = 3, 2
    st = T.step_arrays(n, D, A, seed=C_)
    assert n < 8 or set(st['done_code']) == set(range(8))
    ring, want = T.ring_arrays(C_, D, A, sentinel=True), T.ring_arrays(C_, D, A, sentinel=True)
    O.push_reference(ring, start, final_obs=st['final_obs'] if final else None, **{k: st[k] for k in st if k != 'final_obs'})
    for i in range(n):
        slot = (start + i) % C_
        c = int(st['done_code'][i])
        want['obs'][slot], want['act'][slot], want['rew'][slot] = st['prev_obs'][i], st['action'][i], st['reward'][i]
        want['next_obs'][slot] = st['final_obs'][i] if (c != 0 and final) else st['obs_after'][i]
        want['nonterminal'][slot] = 1.0 if (c == 0 or (c == 7 and final)) else 0.0
    for k in T.RING:
        assert T.bits(ring[k], want[k]), k
    written = np.zeros(C_, bool)
    written[(start + np.arange(n)) % C_] = True
    assert (ring['rew'][~written] == T.SENTINEL).all() and (ring['obs'][~written] == T.SENTINEL).all()
    # each part alone touches its own arrays only
    before, after = T.ring_arrays(C_, D, A, sentinel=True), T.ring_arrays(C_, D, A, sentinel=True)
    O.push_reference(before, start, prev_obs=st['prev_obs'], action=st['action'])
    O.push_reference(after, start, reward=st['reward'], obs_after=st['obs_after'], done_code=st['done_code'], final_obs=st['final_obs'] if final else None)
    assert all(T.bits(before[k], want[k]) for k in ('obs', 'act')) and all((before[k] == T.SENTINEL).all() for k in ('rew', 'next_obs', 'nonterminal'))
    assert all(T.bits(after[k], want[k]) for k in ('rew', 'next_obs', 'nonterminal')) and all((after[k] == T.SENTINEL).all() for k in ('obs', 'act'))


def _splitmix(z):
    M = 2 ** 64 - 1
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


@pytest.mark.parametrize('f', [1, 2, 3, 1000, 2 ** 31 - 1])
def test_sample_index_reference_stays_in_range_and_is_the_formula(f):
    m, G, M = 4096, 0x9E3779B97F4A7C15, 2 ** 64 - 1
    idx = O.sample_index_reference(m, f, seed=12345, draw=7, base=3)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < f and (f < 3 or len(np.unique(idx)) > 1)
    key = _splitmix((12345 + G * 10) & M)                                   # Python integers: the 128-bit product is exact
    assert idx[:64].tolist() == [(_splitmix((key + G * r) & M) * f) >> 64 for r in range(64)]
    assert (O.sample_index_reference(5, 0, 1, 1) == -1).all()


def test_sample_keys():
    m, f = 257, 1000
    a = O.sample_index_reference(m, f, 1, 0)
    assert not np.array_equal(a, O.sample_index_reference(m, f, 2, 0)) and not np.array_equal(a, O.sample_index_reference(m, f, 1, 1))
    assert not np.array_equal(a, O.sample_index_reference(m, f, 1, 0, base=1))
    assert np.array_equal(O.sample_index_reference(m, f, 1, 0, base=1), O.sample_index_reference(m, f, 1, 1, base=0))     # base + draw is what counts
    assert np.array_equal(a, O.sample_index_reference(m, f, 1, 0)) and np.array_equal(a[:100], O.sample_index_reference(100, f, 1, 0))
    assert np.array_equal(O.sample_index_reference(m, f, 2 ** 64 + 1, 2 ** 64), a)                                       # modulo 2^64
    ring = T.ring_arrays(1000, 3, 2, seed=1)
    out = O.sample_reference(ring, 1000, m, 1, 0)
    assert T.bits(out['obs'], ring['obs'][a]) and T.bits(out['qin'], np.concatenate([ring['obs'][a], ring['act'][a]], axis=1))
    assert T.bits(out['rew'], ring['rew'][a]) and out['index'].dtype == np.int32 and out['noise_id'].dtype == np.uint32
    explicit = np.array([0, 999, 1000, -1, 5, 2 ** 40])
    out = O.sample_reference(ring, 1000, 6, indices=explicit)
    assert out['index'].tolist() == [0, 999, -1, -1, 5, -1] and np.isnan(out['qin'][[2, 3, 5]]).all() and np.isnan(out['rew'][[2, 3, 5]]).all()
    assert (out['obs'][[2]].view(np.uint32) == 0x7FC00000).all() and T.bits(out['next_obs'][[0, 1, 4]], ring['next_obs'][[0, 999, 5]])
    assert (O.sample_reference(ring, 0, 4, 1, 0)['index'] == -1).all() and (O.sample_reference(ring, 2000, 4, indices=[1500] * 4)['index'] == -1).all()


@pytest.mark.parametrize('seed,base', [(0, 0), (1, 0), (2024, 5), (2 ** 63 + 11, 2 ** 40)])
def test_sample_index_reference_is_coarsely_uniform(seed, base):
    """2^16 draws at f = 1000: the count in each quarter of [0, f) is binomial(2^16, 1/4) — mean 2^14, standard deviation
    sqrt(2^16 * 1/4 * 3/4) = 110.85 — and lies within 6 of them, 665, of 2^14.  The seeds are fixed: the test is deterministic."""
    n, f = 1 << 16, 1000
    idx = O.sample_index_reference(n, f, seed, 0, base=base)
    bar = int(6 * np.sqrt(n * 0.25 * 0.75))
    assert bar == 665
    counts = np.bincount(idx // 250, minlength=4)
    print('seed %d base %d: quarter counts %s' % (seed, base, counts.tolist()))
    assert counts.sum() == n and (np.abs(counts - (n >> 2)) <= bar).all(), counts


# ---- 5: the rows against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 65, 257, 4096])
def test_critic_reference_against_float64_under_the_derived_bar(m):
    """tests/_offpolicy.py: critic64 writes the derivation out — one term of 2^-24 per fp32 rounding on the path to each output, first
    order, doubled.  Worst ratio seen: 0.41."""
    rows = T.row_inputs(m, seed=m)
    inv_m = np.float32(1) / np.float32(m)
    have = O.critic_reference(*rows, alpha=0.2, gamma=0.99, reward_scale=2.5, inv_m=inv_m)
    want, bars = T.critic64(*rows, alpha=0.2, gamma=0.99, reward_scale=2.5, inv_m=inv_m)
    worst = 0.0
    for k in want:
        err = np.abs(have[k].astype(np.float64) - want[k])
        assert have[k].dtype == np.float32 and (err <= bars[k]).all(), (k, float((err / bars[k]).max()))
        worst = max(worst, float((err / np.maximum(bars[k], 1e-300)).max()))
    print('m %d: worst |x - x64| / bar = %.3f' % (m, worst))
    # log_alpha on the device: alpha = exp_det(log_alpha), 2 ulp of float64's exp
    a = O._alpha_of(None, np.float32(-1.6094379))
    assert abs(float(a) - np.exp(np.float64(np.float32(-1.6094379)))) <= 2 * 2.0 ** -24 * 0.2
    assert T.bits(O.critic_reference(*rows, log_alpha=np.float32(-1.6094379), inv_m=inv_m)['y'], O.critic_reference(*rows, alpha=a, inv_m=inv_m)['y'])


@pytest.mark.parametrize('m', [1, 65, 257, 64 * 256 + 1])
def test_actor_reference_against_float64_under_the_derived_bar(m):
    """tests/_offpolicy.py: actor64.  The cotangents of q1 and q2 are selects and exact; a tie gives everything to q1."""
    q1t, q2t, logp, _r, _n, q1, q2 = T.row_inputs(m, seed=m)
    inv_m = np.float32(1) / np.float32(m)
    have = O.actor_reference(q1, q2, logp, alpha=0.2, inv_m=inv_m, target_entropy=-2.0)
    want, bars = T.actor64(q1, q2, logp, 0.2, inv_m, -2.0)
    for k in want:
        err = np.abs(have[k].astype(np.float64) - want[k])
        assert have[k].dtype == np.float32 and (err <= bars[k]).all(), (k, float(err.max()), float(bars[k].max()))
    assert have['partials'].shape == (64,) and (m > 4 and have['g_q1'][3] == -inv_m and have['g_q2'][3] == 0 or m <= 4)
    assert 'g_log_alpha' not in O.actor_reference(q1, q2, logp, alpha=0.2)
    # the order of S against a plain loop over blocks, lanes and rows
    terms = logp.astype(np.float64) + np.float64(np.float32(-2.0))
    partials = []
    for b in range(64):
        lanes = [0.0] * 256
        for t in range(256):
            for i in range(b * 256 + t, m, 64 * 256):
                lanes[t] += terms[i]
        w = 128
        while w:
            for t in range(w):
                lanes[t] += lanes[t + w]
            w //= 2
        partials.append(lanes[0])
    S = 0.0
    for x in partials:
        S += x
    assert have['partials'].tolist() == partials and have['g_log_alpha'][0] == np.float32(-(S / m))
    # a NaN or an infinity in a row stays in its row, and reaches g_log_alpha through S
    q1b, lpb = q1.copy(), logp.copy()
    q1b[0], lpb[m - 1] = np.nan, np.inf
    bad = O.actor_reference(q1b, q2, lpb, alpha=0.2, inv_m=inv_m, target_entropy=-2.0)
    assert np.isnan(bad['loss'][0]) and bad['g_q2'][0] == -inv_m and not np.isfinite(bad['g_log_alpha'][0])
    if m > 2:
        assert T.bits(bad['loss'][1:m - 1], have['loss'][1:m - 1])


def test_the_minimum_carries_a_nan_from_either_side():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([1, 2, nan, 3, nan, -inf, inf, 0.0], np.float32)
    b = np.array([2, 1, 3, nan, nan, 5, 5, -0.0], np.float32)
    m = O._min_nan(a, b)
    assert np.isnan(m[[2, 3, 4]]).all() and m[[0, 1, 5, 6]].tolist() == [1, 1, -inf, 5] and not np.signbit(m[7])      # a tie keeps the first
    rows = [np.ones(2, np.float32) for _ in range(7)]
    rows[1] = np.array([nan, 1], np.float32)
    out = O.critic_reference(*rows, alpha=0.2)
    assert all(np.isnan(out[k][0]) and np.isfinite(out[k][1]) for k in out)


@pytest.mark.parametrize('count', [1, 255, 4097])
def test_polyak_reference_is_bit_for_bit_a_scalar_loop(count):
    rng = np.random.default_rng(count)
    t, o = rng.standard_normal(count).astype(np.float32), (1e3 * rng.standard_normal(count)).astype(np.float32)
    tau = np.float32(0.005)
    have = O.polyak_reference(t, o, 0.005)
    want = np.array([_libm.fmaf(tau, np.float32(o[i] - t[i]), t[i]) for i in range(count)], np.float32)
    assert have.dtype == np.float32 and T.bits(have, want)
    assert T.bits(O.polyak_reference(t, o, 0.0), t) and T.bits(O.action_grad_reference(np.arange(12, dtype=np.float32).reshape(2, 6), None, 2),
                                                              np.array([[4, 5], [10, 11]], np.float32))
    qin = O.q_pack_reference(np.zeros((2, 5), np.float32), np.ones((2, 3), np.float32), 2 * np.ones((2, 2), np.float32))
    assert qin.tolist() == [[1, 1, 1, 2, 2]] * 2
