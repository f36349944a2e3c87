"""Shared by tests/test_offpolicy_host.py and tests/test_gpu_offpolicy.py (a helper module like _norm.py and _capture.py: pytest does not
collect it, and importing it touches no device): the off-policy library built and bound, the derived bars, the float64 evaluations of the
critic and actor rows, and the inputs of the sweeps."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import offpolicy as O
from tests._epoch import struct_fields  # noqa: F401  (the header's structs as ctypes field lists)
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_offpolicy.h')
KERNELS = ('polyak_kernel', 'q_action_grad_kernel', 'q_pack_kernel', 'replay_push_kernel', 'replay_sample_kernel', 'sac_actor_kernel',
           'sac_alpha_fold_kernel', 'sac_critic_kernel')
ENTRIES = ('eb_replay_push', 'eb_replay_sample', 'eb_q_pack', 'eb_sac_critic', 'eb_sac_actor', 'eb_q_action_grad', 'eb_polyak')
STRUCTS = {'eb_replay_push_args': O.EbReplayPushArgs, 'eb_replay_sample_args': O.EbReplaySampleArgs, 'eb_q_pack_args': O.EbQPackArgs,
           'eb_sac_critic_args': O.EbSacCriticArgs, 'eb_sac_actor_args': O.EbSacActorArgs, 'eb_q_action_grad_args': O.EbQActionGradArgs,
           'eb_polyak_args': O.EbPolyakArgs}
STRUCT_OF = dict(zip(ENTRIES, STRUCTS))
UNIT = ('eb_offpolicy.hip', 'eb_offpolicy.h', 'eb_offpolicy_device.h')
SENTINEL = -77.25
U = 2.0 ** -23
RING = ('obs', 'act', 'rew', 'next_obs', 'nonterminal')


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def fields_of(src, name):
    return struct_fields(src, name, nested={'eb_polyak_segment': O.EbPolyakSegment, 'uint32_t': C.c_uint32, 'uint8_t': C.c_uint8},
                         macros={'EB_OFFPOLICY_MAX_SEGMENTS': O.EB_OFFPOLICY_MAX_SEGMENTS})


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_offpolicy.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, bytes)"""
    path = eb_build.build_offpolicy()
    assert not eb_build.offpolicy_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.offpolicy_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in O.OFFPOLICY_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


def bits(a, b):
    """bit for bit; a NaN equals a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    both_nan = (np.isnan(a) & np.isnan(b)) if a.dtype.kind == 'f' else False
    return bool(((a.view(u) == b.view(u)) | both_nan).all())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def ring_arrays(C_, D, A, seed=0, sentinel=False):
    """a ring of capacity C_ as a dict of float32 arrays: random, or all sentinels"""
    rng = np.random.default_rng(seed)
    shapes = dict(obs=(C_, D), act=(C_, A), rew=(C_,), next_obs=(C_, D), nonterminal=(C_,))
    if sentinel:
        return {k: np.full(s, SENTINEL, np.float32) for k, s in shapes.items()}
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes.items()}


def step_arrays(n, D, A, seed=0):
    """what one env step of n envs leaves behind: prev_obs, action, reward, obs_after, done_code (0 .. 7, every code once n >= 8), final"""
    rng = np.random.default_rng(1000 + seed)
    return dict(prev_obs=rng.standard_normal((n, D)).astype(np.float32), action=rng.standard_normal((n, A)).astype(np.float32),
                reward=rng.standard_normal(n).astype(np.float32), obs_after=rng.standard_normal((n, D)).astype(np.float32),
                done_code=((np.arange(n) + seed) % 8).astype(np.uint8), final_obs=rng.standard_normal((n, D)).astype(np.float32))


def row_inputs(m, seed=0):
    """seven float32 vectors of m rows for the critic and actor rows: q1t, q2t, logp_next, rew, nonterminal (0 / 1), q1, q2"""
    rng = np.random.default_rng(77 + seed)
    q1t, q2t, q1, q2 = (3.0 * rng.standard_normal(m) for _ in range(4))
    if m > 4:
        q2t[3], q2[3] = q1t[3], q1[3]                                       # a tie
    return [np.asarray(x, np.float32) for x in (q1t, q2t, -1.0 + rng.standard_normal(m), 2.0 * rng.standard_normal(m),
                                                (rng.uniform(size=m) < 0.8), q1, q2)]


# ---- the float64 evaluations and the derived bars ----------------------------------------------------------------------------
def critic64(q1t, q2t, logp_next, rew, nonterminal, q1, q2, alpha, gamma, reward_scale, inv_m):
    """eb_sac_critic's formulas in float64 on the float32 inputs (the scalars as their float32 roundings, which both sides share) ->
    (outputs, bars).  Roundings per output, u = 2^-24 each, first order, then DOUBLED for the second-order terms (the bars carry 2^-23):
      e = alpha * logp'            1                        |de| <= u |e|
      v = qm - e                   1                        |dv| <= u |e| + u |v|
      gn = gamma * nt, rs = s * r  1 each                   |d(gn v)| <= |gn| (u |e| + u |v|) + u |gn v|,   |drs| <= u |rs|
      y = fmaf(gn, v, rs)          1                        |dy| <= u (|gn e| + 2 |gn v| + |rs| + |y|)
      d = q - y                    1                        |dd| <= |dy| + u |d|
      loss = (0.5 d) d             1 (0.5 d is exact)       |dloss| <= |d| |dd| + u |loss|
      g = d inv_m                  1                        |dg| <= inv_m |dd| + u |g|"""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    q1t, q2t, logp_next, rew, nonterminal, q1, q2 = map(f, (q1t, q2t, logp_next, rew, nonterminal, q1, q2))
    alpha, gamma, reward_scale, inv_m = (float(np.float32(x)) for x in (alpha, gamma, reward_scale, inv_m))
    e = alpha * logp_next
    v = np.minimum(q1t, q2t) - e
    gn, rs = gamma * nonterminal, reward_scale * rew
    y = gn * v + rs
    bar_y = U * (np.abs(gn * e) + 2 * np.abs(gn * v) + np.abs(rs) + np.abs(y))
    out, bars = dict(y=y), dict(y=bar_y)
    for k, q in (('1', q1), ('2', q2)):
        d = q - y
        bar_d = bar_y + U * np.abs(d)
        out['loss' + k], bars['loss' + k] = 0.5 * d * d, np.abs(d) * bar_d + U * 0.5 * d * d
        out['g_q' + k], bars['g_q' + k] = d * inv_m, inv_m * bar_d + U * np.abs(d * inv_m)
    return out, bars


def actor64(q1, q2, logp, alpha, inv_m, target_entropy):
    """eb_sac_actor's formulas in float64 -> (outputs, bars).  loss = alpha logp - qm: two roundings, |dloss| <= u (|e| + |loss|), doubled;
    g_logp = alpha inv_m: one rounding; g_q1 / g_q2 are selects of -inv_m and 0: exact; g_log_alpha: a double sum of m terms (relative
    m 2^-53 of sum |term|), one division and one rounding to float32."""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    q1, q2, logp = map(f, (q1, q2, logp))
    alpha, inv_m, te = (float(np.float32(x)) for x in (alpha, inv_m, target_entropy))
    m = len(q1)
    e = alpha * logp
    loss = e - np.minimum(q1, q2)
    first = q1 <= q2
    terms = logp + te
    out = dict(loss=loss, g_q1=np.where(first, -inv_m, 0.0), g_q2=np.where(first, 0.0, -inv_m), g_logp=np.full(m, alpha * inv_m),
               g_log_alpha=np.array([-(terms.sum() / m)]))
    bars = dict(loss=U * (np.abs(e) + np.abs(loss)), g_q1=np.zeros(m), g_q2=np.zeros(m), g_logp=np.full(m, U * abs(alpha * inv_m)),
                g_log_alpha=np.array([U * abs(out['g_log_alpha'][0]) + m * 2.0 ** -52 * np.abs(terms).sum() / m]))
    return out, bars
