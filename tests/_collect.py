"""Shared by tests/test_collect_host.py and tests/test_gpu_collect.py (a helper module like _epoch.py and _capture.py: pytest does not
collect it, and importing it touches no device): the collection library built and bound, the synthetic step inputs of the record tests,
rollout buffers cut from the middle of larger allocations, and the parent's collection + head written out."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import collect
from tests._epoch import struct_fields  # noqa: F401  (the header's structs as ctypes field lists)
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_collect.h')
KERNELS = ('collect_begin_kernel', 'collect_episode_log_kernel', 'collect_next_values_kernel', 'collect_record_kernel')
ENTRIES = ('eb_collect_begin', 'eb_collect_record', 'eb_collect_next_values', 'eb_collect_episode_log')
UNIT = ('eb_collect.hip', 'eb_collect.h', 'eb_collect_device.h')
SENTINEL = -77.25
INT_SENTINEL = {np.dtype(np.int32): -77, np.dtype(np.uint8): 0xB3}


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_collect.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, its bytes)"""
    path = eb_build.build_collect()
    assert not eb_build.collect_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.collect_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in collect.COLLECT_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


# ---- synthetic steps ------------------------------------------------------------------------------------------------------------------------
def codes_of(B, t, iteration):
    """done codes of step t: every code 0 .. 7 at every step once B >= 8; env 0 sees 0, 7, 6 and then 7, 6, 5"""
    return ((np.arange(B) + 7 * t + 7 * iteration) % 8).astype(np.uint8)


def step_inputs(B, D, t, iteration):
    """obs [B, D], reward [B], done_code [B], final_obs [B, D] of one synthetic env step"""
    rng = np.random.default_rng(1000 * B + 10 * D + 3 * t + iteration)
    return (rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal(B).astype(np.float32), codes_of(B, t, iteration),
            rng.standard_normal((B, D)).astype(np.float32))


def sentinel_buffers(T, B, D):
    """`collect.buffers` in NumPy with every array at its sentinel, the running state zero: what a kernel does not write stays visible"""
    buf = collect.buffers(T, B, D)
    for k, a in buf.items():
        if k not in ('ep_ret', 'ep_len'):
            a[...] = SENTINEL if a.dtype == np.float32 else INT_SENTINEL[a.dtype]
    return buf


class Slack(object):
    """device copies of a dict of NumPy arrays, each a view into the MIDDLE of a larger allocation with `slack` sentinel elements on both
    sides; host() -> (the arrays back on the host, whether every slack element is as made)"""

    def __init__(self, arrays, slack):
        import torch
        self.slack, self.big, self.views, self.fill = slack, {}, {}, {}
        for k, a in arrays.items():
            fill = SENTINEL if a.dtype == np.float32 or a.dtype == np.float64 else INT_SENTINEL[a.dtype]
            big = torch.full((a.size + 2 * slack,), fill, dtype=getattr(torch, a.dtype.name), device='cuda')
            big[slack:slack + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
            self.big[k], self.fill[k] = big, fill
            self.views[k] = big[slack:slack + a.size].view(a.shape)
            assert self.views[k].is_contiguous() and self.views[k].data_ptr() != big.data_ptr()

    def host(self):
        import torch
        torch.cuda.synchronize()
        out, untouched = {}, True
        for k, big in self.big.items():
            raw = big.cpu().numpy()
            n = raw.size - 2 * self.slack
            out[k] = raw[self.slack:self.slack + n].reshape(tuple(self.views[k].shape)).copy()
            untouched = untouched and bool((raw[:self.slack] == self.fill[k]).all() and (raw[self.slack + n:] == self.fill[k]).all())
        return out, untouched


# ---- the parent's collection + head, as examples/ppo_epoch_loop.py has them ---------------------------------------------------------------------
def parent_collect(env, policy, T, seed, iteration, action_range=1.0):
    """the collection loop of examples/ppo_epoch_loop.py written out — torch copies around sample_actions and env.step — with the codes and
    the final observations kept too -> dict of device tensors (obs [T, B, D], act [T, B, 2], rew, code [T, B], final [T, B, D], last
    [B, D])"""
    import torch
    from env_build_amd.policy_sample import sample_actions
    B, D, dev = env.n_env, env.obs_dim, env.device
    out = dict(obs=torch.empty((T, B, D), device=dev), act=torch.empty((T, B, 2), device=dev), rew=torch.empty((T, B), device=dev),
               code=torch.empty((T, B), dtype=torch.uint8, device=dev), final=torch.empty((T, B, D), device=dev))
    obs = env.obs
    for t in range(T):
        out['obs'][t].copy_(obs.t)
        drawn = sample_actions(policy, out['obs'][t], action_range, seed=seed, counter=iteration * T + t, want=())
        out['act'][t].copy_(drawn['actions'].t)
        obs, reward, _done, info = env.step(drawn['actions'])
        out['rew'][t].copy_(reward.t)
        out['code'][t].copy_(env.done_code)
        out['final'][t].copy_(info['final_observation'].t)
    out['last'] = obs.t.clone()
    return out
