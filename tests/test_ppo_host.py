"""CPU (-m "not gpu"): the PPO family (include/envbuild_ppo.h, env_build_amd.ppo) — its header against the module's own binding table
and argument structs, the built library's exports and device-free refusals, the NumPy restatement of the surrogate row against torch
float64 autograd of the expression examples/ppo_env_loop.py writes, the float32 restatement against the float64 one, the restatement
of generalised advantage estimation against a torch float32 transcription of the example's loop bit for bit and against the closed
form, and NaN handling."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import policy_logp as pl
from env_build_amd import ppo
from tests._helpers import ROOT, oracle_lib
from tests._ppo import example_loop, sampled, within      # test_policy_logp_host.py's inputs (log-std in [-2, 1], |x| <= 5.3) and bar

HEADER = os.path.join(ROOT, 'include', 'envbuild_ppo.h')
KERNELS = ('ppo_surrogate_kernel', 'ppo_surrogate_logits_kernel', 'gae_kernel')
RANGES = (1.0, 0.5, None)
CLIP, ENT_COEF = 0.2, 0.01
ADV_NORM = (0.3, 1.7)                                          # (mean, 1 / std)
TARGETS = (0.6, 0.95, 1.5)                                     # ratios below lo = 0.8, inside, above hi = 1.2


# ---- 1: the header is what the module binds ---------------------------------------------------------------------------------------------
def ctype_of(decl):
    decl = decl.replace('const ', '').strip()
    if decl.endswith('*'):
        return C.c_void_p
    return {'int32_t': C.c_int32, 'float': C.c_float, 'double': C.c_double}[decl]


def struct_fields(src, name):
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        if not decl.strip():
            continue
        first, *more = [p.strip() for p in decl.split(',')]
        m = re.match(r'(.*?)(\w+)$', first)
        fields.append((m.group(2), ctype_of(m.group(1))))
        fields += [(p, ctype_of(m.group(1))) for p in more]
    return fields


def test_header_declares_what_the_module_binds():
    text = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = sorted(set(re.findall(r'\bint\s+(eb_[a-z0-9_]+)\s*\(', src)))
    assert names == sorted(ppo.PPO_PROTOTYPES) == ['eb_gae', 'eb_ppo_abi_version', 'eb_ppo_surrogate', 'eb_ppo_surrogate_from_logits',
                                                   'eb_ppo_surrogate_supported']
    kinds = {'eb_mlp': C.c_void_p, 'int32_t*': C.POINTER(C.c_int32), 'const eb_ppo_args*': C.POINTER(ppo.EbPpoArgs),
             'const eb_gae_args*': C.POINTER(ppo.EbGaeArgs)}
    for name, (res, args) in ppo.PPO_PROTOTYPES.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m and res is C.c_int, name
        params = [a.strip() for a in m.group(1).split(',') if a.strip() != 'void']
        assert [kinds[re.sub(r'\s*\w+$', '', p)] for p in params] == args, name
        assert not any(re.search(r'\bstream$', p) for p in params), name
    assert not re.search(r'\bint\s+eb_\w+\s*\([^)]*void\s*\*\s*stream[^)]*\)', src)      # the stream is a field of the struct
    assert int(re.search(r'#define EB_PPO_ABI_VERSION (\d+)', text).group(1)) == ppo.EB_PPO_ABI_VERSION == 1
    for name, struct in (('eb_ppo_args', ppo.EbPpoArgs), ('eb_gae_args', ppo.EbGaeArgs)):
        assert struct_fields(src, name) == list(struct._fields_), name
        assert struct._fields_[-1] == ('stream', C.c_void_p)
    for words in ('bit for bit', 'exp_det', 'eb_mlp_backward(head = 0)', 'ALWAYS exactly one launch', 'ppo_reference', 'gae_reference',
                  '1.4189385332f', 'AT CALL TIME', 'tests/test_stream_census.py', 'blocked', 'the ratio', 'HALF', 'never reads it',
                  "info['final_observation']", 'examples/ppo_env_loop.py'):
        assert words in text, words


def test_the_family_tables_are_untouched():
    assert not set(ppo.PPO_PROTOTYPES) & set(_capi.PROTOTYPES)
    for row in _capi.FAMILIES.values():
        assert not set(ppo.PPO_PROTOTYPES) & set(row[5])
    assert not set(ppo.PPO_PROTOTYPES) & set(pl.POLICY_LOGP_PROTOTYPES)
    for header in ('envbuild.h', 'envbuild_policy_logp.h', 'envbuild_policy_sample.h'):
        text = open(os.path.join(ROOT, 'include', header)).read()
        assert 'eb_ppo' not in text and 'eb_gae' not in text
    import env_build_amd
    assert not [n for n in dir(env_build_amd) if n in ppo.__all__]      # the package surface is the logp family's: the module itself


@pytest.fixture(scope='module')
def hip_library():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    lib.eb_last_error.restype = C.c_char_p
    for name, (res, args) in ppo.PPO_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, open(lib_path, 'rb').read()


def test_the_library_exports_the_entries_and_the_kernels(hip_library):
    lib, blob = hip_library
    assert lib.eb_ppo_abi_version() == 1
    for kernel in KERNELS:
        assert kernel.encode() in blob, kernel
    public = os.path.join('..', '..', 'include', 'envbuild_ppo.h')
    assert 'eb_ppo.hip' in eb_build.SOURCES
    assert {'eb_ppo.h', 'eb_ppo_device.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not [f for f in files if 'ppo' in f]
    unit = open(os.path.join(eb_build.CSRC, 'eb_ppo.hip')).read() + open(os.path.join(eb_build.CSRC, 'eb_ppo_device.h')).read()
    assert set(re.findall(r'#include "(eb_[a-z0-9_]+\.h)"', unit)) <= set(eb_build.HEADERS)


def test_refusals_need_no_device_and_name_their_entry(hip_library):
    lib, _ = hip_library
    seven = C.c_int32(7)
    buf = (C.c_float * 8)()
    p = C.addressof(buf)
    nan, inf = float('nan'), float('inf')

    def args(n=4, out_dim=2, action_range=1.0, clip=0.2, ent_coef=0.0, scale=1.0, **kw):
        full = dict(obs=p, logits=p, actions=p, logp_old=p, adv=p, logp=p, g_logits=p)
        full.update(kw)
        return C.byref(ppo.EbPpoArgs(n=n, out_dim=out_dim, action_range=action_range, clip=clip, ent_coef=ent_coef, scale=scale, **full))

    def gargs(T=2, n=2, gamma=0.99, lam=0.95, **kw):
        full = dict(rewards=p, values=p, v_last=p, nonterminal=p, adv=p, ret=p)
        full.update(kw)
        return C.byref(ppo.EbGaeArgs(T=T, n=n, gamma=gamma, lam=lam, **full))

    one = 'eb_ppo_surrogate_from_logits'
    calls = [
        ('eb_ppo_surrogate_supported', (None, C.byref(seven))),
        ('eb_ppo_surrogate', (None, args())),
        ('eb_ppo_surrogate', (None, None)),
        (one, (None,)),
        (one, (args(logits=None),)), (one, (args(actions=None),)), (one, (args(logp_old=None),)), (one, (args(adv=None),)),
        (one, (args(logp=None),)),
        (one, (args(n=1, out_dim=3),)), (one, (args(n=1, out_dim=34),)), (one, (args(n=1, out_dim=0),)), (one, (args(n=-1),)),
        (one, (args(n=1, action_range=nan),)), (one, (args(n=1, clip=nan),)), (one, (args(n=1, clip=-0.1),)),
        (one, (args(n=1, ent_coef=nan),)), (one, (args(n=1, scale=nan),)),
        ('eb_gae', (None,)),
        ('eb_gae', (gargs(T=0),)), ('eb_gae', (gargs(T=65536),)), ('eb_gae', (gargs(n=-1),)),
        ('eb_gae', (gargs(gamma=nan),)), ('eb_gae', (gargs(lam=nan),)), ('eb_gae', (gargs(gamma=inf),)), ('eb_gae', (gargs(lam=-inf),)),
        ('eb_gae', (gargs(rewards=None),)), ('eb_gae', (gargs(values=None),)), ('eb_gae', (gargs(nonterminal=None),)),
        ('eb_gae', (gargs(adv=None),)), ('eb_gae', (gargs(v_last=None),)),
    ]
    for name, a in calls:
        assert getattr(lib, name)(*a) == -1, name
        assert lib.eb_last_error().startswith(name.encode() + b':'), (name, lib.eb_last_error())
    assert seven.value == 7 and all(v == 0.0 for v in buf)
    # n = 0 is a no-op that needs no pointer and no device
    assert lib.eb_ppo_surrogate_from_logits(C.byref(ppo.EbPpoArgs(n=0, out_dim=2, action_range=1.0, clip=0.2, scale=1.0))) == 0
    assert lib.eb_gae(C.byref(ppo.EbGaeArgs(T=3, n=0, gamma=0.99, lam=0.95))) == 0


def test_a_library_without_the_entries_is_refused_by_header_name():
    api = oracle_lib()
    assert api.backend == 'oracle'
    with pytest.raises(_capi.EbError) as e:
        ppo.bind(api)
    assert 'envbuild_ppo.h' in str(e.value) and 'eb_gae' in str(e.value)


# ---- 2, 3: the surrogate row against torch float64 autograd, and float32 against float64 ------------------------------------------------
def surrogate_case(act_dim, action_range):
    """that file's logits and sampled actions (24 rows); logp_old placed so that row k's ratio is TARGETS[k % 3] and its normalised
    advantage has the sign (-1) ** (k // 3); row 0: logp_old is the float32 restatement's own logp, r == 1 there"""
    logits, _, actions, _ = sampled(act_dim, action_range)
    n = len(logits)
    rng = np.random.default_rng(77 + act_dim)
    logp32 = pl.policy_logp_reference(logits, actions, action_range)[0]
    logp_old = (logp32.astype(np.float64) - np.log(np.array(TARGETS)[np.arange(n) % 3])).astype(np.float32)
    logp_old[0] = logp32[0]
    sign = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    adv = (ADV_NORM[0] + sign * (0.2 + np.abs(rng.standard_normal(n))) / ADV_NORM[1]).astype(np.float32)
    return logits, actions, logp_old, adv


def torch_yardstick(logits, actions, logp_old, adv, action_range, clip, ent_coef, adv_norm, own_logp_old=False):
    """float64: the expression of examples/ppo_env_loop.py — TransformedDistribution.log_prob, exp, clamp, min, mean, the entropy — with
    the advantage normalised by adv_norm, and autograd of the loss with respect to the logits"""
    import torch
    from torch import distributions as D
    y = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    a = torch.tensor(np.asarray(actions, np.float64))
    act_dim = y.shape[1] // 2
    dist = D.Independent(D.Normal(y[:, :act_dim], y[:, act_dim:].exp()), 1)
    if action_range is not None:
        dist = D.TransformedDistribution(dist, [D.transforms.TanhTransform(), D.transforms.AffineTransform(0.0, float(action_range))])
    logp = dist.log_prob(a)
    old = logp.detach().clone() if own_logp_old else torch.tensor(np.asarray(logp_old, np.float64))
    A = torch.tensor(np.asarray(adv, np.float64))
    if adv_norm is not None:
        A = (A - float(adv_norm[0])) * float(adv_norm[1])
    ratio = (logp - old).exp()
    surr = torch.min(ratio * A, ratio.clamp(1.0 - clip, 1.0 + clip) * A)
    entropy = (y[:, act_dim:] + 0.5 * math.log(2.0 * math.pi * math.e)).sum(1).mean()
    loss = -surr.mean() - ent_coef * entropy
    loss.backward()
    return dict(logp=logp.detach().numpy(), ratio=ratio.detach().numpy(), surr=surr.detach().numpy(), loss=float(loss.detach()),
                g_logits=y.grad.numpy())


def regions(ratio, A, clip):
    lo, hi = 1.0 - clip, 1.0 + clip
    where = np.where(ratio < lo, 0, np.where(ratio > hi, 2, 1))
    return {(int(w), bool(s)) for w, s in zip(where, A > 0)}


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float64_restatement_equals_torch_autograd_of_the_examples_expression(act_dim, action_range):
    logits, actions, logp_old, adv = surrogate_case(act_dim, action_range)
    want = torch_yardstick(logits, actions, logp_old, adv, action_range, CLIP, ENT_COEF, ADV_NORM)
    got = ppo.ppo_reference(logits, actions, logp_old, adv, action_range, CLIP, ENT_COEF, adv_norm=ADV_NORM, dtype=np.float64)
    assert all(got[k].dtype == np.float64 for k in ('logp', 'ratio', 'surr', 'g_logits'))
    # below lo, inside and above hi, each with both signs of the advantage
    assert regions(got['ratio'], got['A'], CLIP) == {(w, s) for w in (0, 1, 2) for s in (False, True)}
    assert abs(got['ratio'][0] - 1.0) < 1e-5
    what = 'act_dim %d, action_range %r' % (act_dim, action_range)
    for k in ('logp', 'ratio', 'surr', 'g_logits'):
        within(got[k], want[k], 1e-12, '%s, %s' % (k, what))
    assert abs(got['loss'] - want['loss']) <= 1e-12 * max(abs(want['loss']), np.abs(want['surr']).max())
    # blocked rows have no surrogate gradient: what is left on them is the entropy bonus
    blocked = ((got['ratio'] < 1 - CLIP) & (got['A'] < 0)) | ((got['ratio'] > 1 + CLIP) & (got['A'] > 0))
    assert blocked.any() and (got['g_lp'][blocked] == 0).all() and (got['g_lp'][~blocked] != 0).all()
    assert np.allclose(want['g_logits'][blocked][:, :act_dim], 0.0, rtol=0, atol=0)


@pytest.mark.parametrize('clip', [0.2, 0.0])
def test_the_ties_of_blocked_are_torchs(clip):
    """r == 1 exactly (the first pass of every batch): both products are equal, torch.min splits the cotangent in halves and the clamp
    passes on the closed interval — lo == hi == 1 with clip 0 included — so the gradient is the full one, as `blocked` has it.
    A == 0 outside the interval: zero on both sides."""
    logits, actions, _, adv = surrogate_case(2, 1.0)
    adv = adv.astype(np.float64)
    adv[5] = ADV_NORM[0]                                             # A == 0 after the normalisation
    ref = ppo.ppo_reference(logits, actions, np.zeros(len(adv)), adv, 1.0, clip, ENT_COEF, adv_norm=ADV_NORM, dtype=np.float64)
    want = torch_yardstick(logits, actions, None, adv, 1.0, clip, ENT_COEF, ADV_NORM, own_logp_old=True)
    got = ppo.ppo_reference(logits, actions, ref['logp'], adv, 1.0, clip, ENT_COEF, adv_norm=ADV_NORM, dtype=np.float64)
    assert (got['ratio'] == 1.0).all() and (want['ratio'] == 1.0).all() and got['A'][5] == 0.0
    n = len(adv)
    assert np.array_equal(got['g_lp'], (-1.0 / n) * got['A'])           # the full gradient on every row
    within(got['g_logits'], want['g_logits'], 1e-12, 'g_logits at r == 1, clip %g' % clip)
    # A == 0 outside: logp_old moved so that r = 2
    old = ref['logp'] - math.log(2.0)
    want = torch_yardstick(logits, actions, old, adv, 1.0, clip, 0.0, ADV_NORM)
    got = ppo.ppo_reference(logits, actions, old, adv, 1.0, clip, 0.0, adv_norm=ADV_NORM, dtype=np.float64)
    assert got['g_lp'][5] == 0.0 and (got['g_logits'][5] == 0.0).all() and (want['g_logits'][5] == 0.0).all()
    within(got['g_logits'], want['g_logits'], 1e-12, 'g_logits at r == 2, clip %g' % clip)


# float32 against float64: tests/test_policy_logp_host.py's bar, 1e-5 of each tensor's maximum.  The ratio is one exponential of a
# float32 DIFFERENCE of two log-probabilities, so it inherits the absolute error of logp (a sum of act_dim terms) as a relative one, and
# surr, the loss and g_logits inherit the ratio's.  Measured on these 12 cases: ratio 3.9e-6 of a maximum of 1.5 and g_logits 3.9e-6 of
# a maximum of 1.48 at worst (act_dim 16, action_range 0.5), 2.6e-6 of the maximum: the bar holds as it is.
BAR32 = {'logp': 1e-5, 'ratio': 1e-5, 'surr': 1e-5, 'g_logits': 1e-5}


@pytest.mark.parametrize('action_range', RANGES)
@pytest.mark.parametrize('act_dim', [1, 2, 3, 16])
def test_float32_restatement_is_within_the_bar_of_float64(act_dim, action_range):
    logits, actions, logp_old, adv = surrogate_case(act_dim, action_range)
    kw = dict(adv_norm=ADV_NORM)
    want = ppo.ppo_reference(logits, actions, logp_old, adv, action_range, CLIP, ENT_COEF, dtype=np.float64, **kw)
    got = ppo.ppo_reference(logits, actions, logp_old, adv, action_range, CLIP, ENT_COEF, dtype=np.float32, **kw)
    assert got['ratio'][0] == 1.0                                      # logp_old is this restatement's own logp there
    assert np.array_equal(got['g_lp'] == 0, want['g_lp'] == 0)         # the same rows are blocked
    for k, bar in BAR32.items():
        assert got[k].dtype == np.float32
        within(got[k], want[k], bar, '%s, act_dim %d, action_range %r' % (k, act_dim, action_range))
    assert abs(got['loss'] - want['loss']) <= BAR32['surr'] * np.abs(want['surr']).max()


# ---- 4: generalised advantage estimation ---------------------------------------------------------------------------------------------------
def gae_case(T, n=7, seed=0):
    rng = np.random.default_rng(100 * T + seed)
    rewards = rng.standard_normal((T, n)).astype(np.float32)
    values = rng.standard_normal((T, n)).astype(np.float32)
    v_last = rng.standard_normal(n).astype(np.float32)
    live = (rng.uniform(size=(T, n)) > 0.2).astype(np.float32)
    live[0, 0] = 0.0
    live[T - 1, n - 1] = 0.0
    return rewards, values, v_last, live


@pytest.mark.parametrize('gamma, lam', [(0.99, 0.95), (0.9, 0.8), (1.0, 1.0), (0.997, 0.3)])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 8, 33])      # window remainders 1, 2, 3 of GAE_WIN = 4, one and two exact windows, many
def test_gae_float32_restatement_is_the_examples_loop_bit_for_bit(T, gamma, lam):
    rewards, values, v_last, live = gae_case(T)
    want = example_loop(rewards, values, v_last, live, gamma, lam)
    got = ppo.gae_reference(rewards, values, v_last, live, gamma, lam)
    assert got[0].dtype == got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_gae_float64_restatement_is_the_closed_form_and_terminals_cut():
    T, n, gamma, lam = 33, 5, 0.99, 0.95
    rewards, values, v_last, _ = gae_case(T, n)
    live = np.ones((T, n), np.float32)
    adv, ret = ppo.gae_reference(rewards, values, v_last, live, gamma, lam, dtype=np.float64)
    r, v = rewards.astype(np.float64), np.concatenate([values, v_last[None]]).astype(np.float64)
    delta = r + gamma * v[1:] - v[:-1]
    want = np.stack([sum((gamma * lam) ** k * delta[t + k] for k in range(T - t)) for t in range(T)])
    assert np.abs(adv - want).max() <= 1e-12 * np.abs(want).max() and np.abs(ret - (want + v[:-1])).max() <= 1e-12 * np.abs(want).max()
    # a terminal at step t cuts the bootstrap and the carry: adv[t] = r[t] - v[t], and nothing at or before t sees what follows
    t = 20
    live[t, 2] = 0.0
    cut, _ = ppo.gae_reference(rewards, values, v_last, live, gamma, lam, dtype=np.float64)
    assert cut[t, 2] == r[t, 2] - v[t, 2]
    other = rewards.copy()
    other[t + 1:, 2] += 5.0
    moved, _ = ppo.gae_reference(other, values, v_last, live, gamma, lam, dtype=np.float64)
    assert np.array_equal(moved[:t + 1, 2], cut[:t + 1, 2]) and not np.array_equal(moved[t + 1:, 2], cut[t + 1:, 2])
    assert np.array_equal(cut[:, [0, 1, 3, 4]], adv[:, [0, 1, 3, 4]])
    # nonterminal = 1, carry = 0 with next_values: a truncation bootstraps from the given value and does not carry
    live[t, 2] = 1.0
    carry = live.copy()
    carry[t, 2] = 0.0
    nv = np.concatenate([values[1:], v_last[None]]).astype(np.float32)
    nv[t, 2] = 3.25                                                   # the value of the final observation
    trunc, _ = ppo.gae_reference(rewards, values, None, live, gamma, lam, next_values=nv, carry=carry, dtype=np.float64)
    assert trunc[t, 2] == (r[t, 2] + gamma * 3.25) - v[t, 2]
    assert np.array_equal(trunc[:, [0, 1, 3, 4]], adv[:, [0, 1, 3, 4]]) and np.array_equal(trunc[t + 1:, 2], adv[t + 1:, 2])


# ---- 5: NaN handling -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_a_nan_poisons_its_own_row_and_a_zero_advantage_outside_is_blocked(dtype):
    logits, actions, logp_old, adv = surrogate_case(2, 1.0)
    adv, logp_old = adv.copy(), logp_old.copy()
    adv[4] = np.nan
    logp_old[7] = np.nan
    adv[9] = 0.0                                                     # row 9: k % 3 == 0, ratio 0.6 < lo
    adv[11] = -0.0                                                   # row 11: ratio 1.5 > hi
    out = ppo.ppo_reference(logits, actions, logp_old, adv, 1.0, CLIP, ENT_COEF, dtype=dtype)
    for row in (4, 7):
        assert np.isnan(out['surr'][row]) and np.isnan(out['g_lp'][row]) and np.isnan(out['g_logits'][row]).all(), row
    assert np.isnan(out['ratio'][7]) and np.isfinite(out['ratio'][4])
    clean = np.ones(len(adv), bool)
    clean[[4, 7]] = False
    for k in ('logp', 'ratio', 'surr', 'ent', 'g_lp', 'g_logits'):
        assert np.isfinite(out[k][clean]).all(), k
    assert np.isfinite(out['logp']).all() and np.isfinite(out['ent']).all()
    for row in (9, 11):
        assert out['g_lp'][row] == 0.0 and not (1 - CLIP <= out['ratio'][row] <= 1 + CLIP)
        assert np.array_equal(out['g_logits'][row, :2], [0.0, 0.0])
        assert np.array_equal(out['g_logits'][row, 2:], np.full(2, -(dtype(1.0 / len(adv)) * dtype(ENT_COEF)), dtype))
