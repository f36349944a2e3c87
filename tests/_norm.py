"""Shared by tests/test_norm_host.py and tests/test_gpu_norm.py (a helper module like _collect.py and _capture.py: pytest does not collect
it, and importing it touches no device): the normalisation library built and bound, the derived bars, the inputs of the sweeps, the G22
fixture and its replay through any engine — the NumPy restatements or the device entries."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import norm
from tests._epoch import struct_fields  # noqa: F401  (the header's structs as ctypes field lists)
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_norm.h')
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g22_norm.npz')
KERNELS = ('norm_apply_kernel', 'norm_fold_kernel', 'norm_partial_kernel')
ENTRIES = ('eb_norm_update', 'eb_norm_apply')
UNIT = ('eb_norm.hip', 'eb_norm.h', 'eb_norm_device.h')
SENTINEL = -77.25
U = 2.0 ** -23


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_norm.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, its bytes)"""
    path = eb_build.build_norm()
    assert not eb_build.norm_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.norm_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in norm.NORM_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


# ---- the derived bars -----------------------------------------------------------------------------------------------------
def obs_bar(mean, den, y64):
    """|y - y64| <= 2^-23 (|mean| / den + 4 |y64|): one rounding of the mean amplified by 1 / den, two roundings in den_f, one in the
    subtraction, one in the division — 2^-24 each — then doubled.  The clip is 1-Lipschitz and needs no term."""
    return U * (np.abs(mean) / den + 4.0 * np.abs(y64))


def rew_bar(r64):
    """the division carries no mean term"""
    return U * 4.0 * np.abs(r64)


class State64(object):
    """the same formulas evaluated in float64 with NumPy's own mean and var: the yardstick of the sweeps"""

    def __init__(self, D, epsilon=1e-8):
        self.mean, self.var, self.count, self.eps = np.zeros(D), np.ones(D), 1e-4, epsilon

    def update(self, x):
        x = np.asarray(x, np.float64).reshape(-1, self.mean.size)
        bm, bv, n = x.mean(axis=0), x.var(axis=0), x.shape[0]
        delta, tot = bm - self.mean, self.count + n
        M2 = self.var * self.count + bv * n + delta * delta * self.count * n / tot
        self.mean, self.var, self.count = self.mean + delta * n / tot, M2 / tot, tot

    @property
    def den(self):
        return np.sqrt(self.var + self.eps)

    def apply(self, x, clip):
        return np.clip((np.asarray(x, np.float64) - self.mean) / self.den, -clip, clip)

    def apply_reward(self, r, clip):
        return np.clip(np.asarray(r, np.float64) / self.den[0], -clip, clip)


def sweep_batch(B, D, k, spread=True):
    """batch k of the sweep at (B, D): float32 [B, D] with |mean| <= 10^3 and std from 0 (column 0 is constant once D > 1) to 10^2"""
    rng = np.random.default_rng(100000 + 1000 * D + B)
    mean = rng.uniform(-1e3, 1e3, D) if spread else rng.uniform(-3, 3, D)
    std = 10.0 ** rng.uniform(-3, 2, D) if spread else np.ones(D)
    if D > 1:
        std[0] = 0.0
    rng = np.random.default_rng(7 * B + 13 * D + k)
    return (mean + std * rng.standard_normal((B, D))).astype(np.float32)


# ---- the fixture through an engine --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


class HostEngine(object):
    """the NumPy restatements behind the few calls the replays make; tests/test_gpu_norm.py has the device's twin"""

    def state(self, D, epsilon):
        return norm.HostState(D, epsilon)

    def zeros(self, n):
        return np.zeros(n, np.float32)

    def update_obs(self, state, x):
        norm.update_reference(state, x)

    def apply_obs(self, state, x, clip):
        return norm.apply_reference(state, x, clip)

    def step_reward(self, state, reward, ret_run, gamma, clip, done):
        """process_rew: the return part of the update, then the reward part of the apply -> the normalised rewards"""
        norm.update_return_reference(state, reward, ret_run, gamma)
        return norm.apply_reward_reference(state, reward, clip, done, ret_run)

    def host(self, state):
        return state

    def array(self, a):
        return np.asarray(a)


def den64(state):
    """sqrt(var + epsilon) of a HostState's float64 statistics"""
    D = state.D
    return np.sqrt(state.stat[D:2 * D] + state.epsilon)


def replay_obs(engine, B, D):
    """G22 (1) through `engine` -> (largest |y - y_ref| / bar, where bar = |y_ref - y64| + obs_bar: the triangle inequality, no margin)"""
    g, key = golden(), 'obs_B%d_D%d/' % (B, D)
    x, clip = g[key + 'x'], float(g[key + 'clip'])
    state = engine.state(D, float(g['epsilon']))
    worst = 0.0
    for k in range(x.shape[0]):
        engine.update_obs(state, x[k])
        y = engine.array(engine.apply_obs(state, x[k], clip))
        h = engine.host(state)
        bar = np.abs(g[key + 'y_ref'][k].astype(np.float64) - g[key + 'y64'][k]) + obs_bar(h.stat[:D], den64(h), g[key + 'y64'][k])
        err = np.abs(y.astype(np.float64) - g[key + 'y_ref'][k])
        assert y.dtype == np.float32 and (err <= bar).all(), (key, k, float((err / bar).max()))
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    h = engine.host(state)
    assert h.stat[2 * D] == float(g[key + 'count_64']) and np.allclose(h.stat[:D], g[key + 'mean_64'], rtol=1e-12, atol=1e-12)
    assert np.allclose(h.stat[D:2 * D], g[key + 'var_64'], rtol=1e-9, atol=1e-15)
    return worst


def replay_rewards(engine, which):
    """G22 (2) ('rew1': one env, n = 1 per step) or (3) ('rewB') through `engine` under the triangle bar; the running return is held to the
    reference's float32 recursion bit for bit — it is the same two fp32 operations"""
    g = golden()
    rew, done = g[which + '/rew'], g[which + '/done']
    steps = rew.shape[0]
    rew, done = rew.reshape(steps, -1), done.reshape(steps, -1)
    state, ret_run = engine.state(1, float(g['epsilon'])), engine.zeros(rew.shape[1])
    worst = 0.0
    for t in range(steps):
        r = engine.array(engine.step_reward(state, rew[t], ret_run, float(g['gamma']), 10.0, done[t]))
        want, r64 = g[which + '/r_ref'].reshape(steps, -1)[t], g[which + '/r64'].reshape(steps, -1)[t]
        bar = np.abs(want.astype(np.float64) - r64) + rew_bar(r64)
        err = np.abs(r.astype(np.float64) - want)
        assert r.dtype == np.float32 and (err <= bar).all(), (which, t, float((err / bar).max()))
        worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        if which == 'rew1':                                                  # ret_rms after every step
            # (the yardstick's recursion is float64, ours the reference's float32 one: at most 2 roundings of 2^-24 per step on R, so
            #  steps * 2 * 2^-24 relative to the returns' own size — |mean| + std for the mean, twice that, relatively, for the variance)
            h, want = engine.host(state), g['rew1/rms64'][t]
            size = np.array([abs(want[0]) + np.sqrt(want[1]), 2.0 * want[1], 0.0])
            assert (np.abs(h.stat - want) <= steps * 2 * 2.0 ** -24 * size).all(), (t, h.stat, want)
    final = engine.array(ret_run)
    if which == 'rewB':
        assert np.array_equal(final, g['rewB/ret_ref']) and (final[done[-1] != 0] == 0).all()
    return worst
