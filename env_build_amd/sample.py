"""S perturbed action tapes per env drawn, rolled out, scored and averaged in ONE launch: rollout_tape_samples.

The cost of an open-loop tape is non-convex (the collision discs, DAM:218-229), so a descent ends in the basin it starts in.  A
sampling planner (MPPI / CEM) takes hundreds of perturbed tapes per scene and a soft-min average of them, and needs no gradient.
eb_rollout_tape_sample (include/envbuild_sample.h, csrc/eb_rollout_tape_sample.hip) does one such step in one launch: the scene's
vehicle records advance once per env, the perturbations are a pure function of (seed, counter, env id, sample, step, component) and
never exist in memory, and the reduction over an env's samples stays in its block.

    out = rollout_tape_samples(model, obses, nominal, 256, seed=0, counter=k, sigma=(0.3, 0.3), beta=0.7, lam=1.0, ref_indexes=ref)
    out['cost'] [S, B], out['best_tape'] [H, B, 2], out['best_cost'] [B], out['best_index'] [B], out['mean_tape'] [H, B, 2]

sample_tapes_reference / softmin_mean_reference restate the noise, the samples and the soft-min mean in NumPy / torch: they are the
definition a reader checks the header against, and what the tests compare the kernel with.  fp32 state only; no CPU path and no
fall-back to chunks of eb_rollout_tape_cand: without the HIP library's entry rollout_tape_samples raises.
"""
import ctypes as C
import math

import numpy as np
import torch

from ._tape_args import check_rows, five_weights, need_fp32, path_args
from .dynamics_and_models import _dev, _stream
from .mpc import DEFAULT_WEIGHTS, first_minimum

__all__ = ['rollout_tape_samples', 'tape_sample_max', 'sample_tapes_reference', 'sample_noise_reference', 'softmin_mean_reference']

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_U64 = (1 << 64) - 1


def _splitmix64(z):
    """csrc/eb_env_device.h:253-258 on a uint64 array (arithmetic modulo 2^64)"""
    with np.errstate(over='ignore'):
        z = z + _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _u01(key, idx):
    """csrc/eb_env_device.h:260-262: the top 24 bits of splitmix64(key + GOLDEN * idx) -> [0, 1) in float32"""
    with np.errstate(over='ignore'):
        return (_splitmix64(key + _GOLDEN * idx) >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def sample_noise_reference(env_ids, n_samples, horizon, seed, counter, beta=0.0):
    """eps [S, H, B, 2] float32 (NumPy) of include/envbuild_sample.h, bit for bit; eps[0] is zero (sample 0 is the nominal).
    env_ids: B non-negative ints below 2^32."""
    ids = np.asarray(env_ids, dtype=np.int64).astype(np.uint64) & np.uint64(0xffffffff)
    S, H, B = int(n_samples), int(horizon), ids.shape[0]
    key = _splitmix64(np.array([(int(seed) + 0x9E3779B97F4A7C15 * int(counter)) & _U64], dtype=np.uint64))[0]
    with np.errstate(over='ignore'):
        s = np.arange(S, dtype=np.uint64).reshape(S, 1, 1, 1)
        t = np.arange(H, dtype=np.uint64).reshape(1, H, 1, 1)
        a = np.arange(2, dtype=np.uint64).reshape(1, 1, 1, 2)
        i = ids.reshape(1, 1, B, 1)
        idx = np.uint64(4) * (a + np.uint64(2) * (t + np.uint64(H) * (i * np.uint64(S) + s)))
        u = [_u01(key, idx + np.uint64(j)) for j in range(4)]
    xi = (((u[0] + u[1]) + (u[2] + u[3])) - np.float32(2.0)) * np.float32(1.7320508)
    b32 = np.float32(beta)
    gain = np.float32(math.sqrt(1.0 - float(b32) * float(b32)))
    eps = np.empty_like(xi)
    eps[:, 0] = xi[:, 0]
    for k in range(1, H):
        eps[:, k] = b32 * eps[:, k - 1] + gain * xi[:, k]
    eps[0] = 0.0
    return eps


def _clamp(x):
    """x < -1 ? -1 : x > 1 ? 1 : x — a NaN stays a NaN (torch.clamp's rule)"""
    return x.clamp(-1.0, 1.0)


def sample_tapes_reference(nominal, n_samples, seed, counter, sigma, beta=0.0, env_ids=None):
    """The tapes eb_rollout_tape_sample scores: nominal [H, B, 2] (any device and float dtype) -> samples [S, H, B, 2] of the same
    device and dtype.  Sample 0 is clamp(nominal); sample s >= 1 is clamp(nominal + sigma[a] * eps) with eps the float32 noise of
    sample_noise_reference, every operation one rounding in nominal's dtype: in float32 these are the kernel's bits."""
    H, B = nominal.shape[0], nominal.shape[1]
    ids = np.arange(B) if env_ids is None else (env_ids.detach().cpu().numpy() if torch.is_tensor(env_ids) else np.asarray(env_ids))
    eps = torch.from_numpy(sample_noise_reference(ids, n_samples, H, seed, counter, beta)).to(device=nominal.device, dtype=nominal.dtype)
    sig = torch.tensor([float(np.float32(sigma[0])), float(np.float32(sigma[1]))], dtype=nominal.dtype, device=nominal.device)
    out = nominal.unsqueeze(0) + sig * eps
    out[0] = nominal
    return _clamp(out)


def softmin_mean_reference(samples, cost, lam):
    """The soft-min average of include/envbuild_sample.h in samples' dtype: samples [S, H, B, 2], cost [S, B] ->
    (mean_tape [H, B, 2], best_index [B]).  w_s = exp(-(cost_s - cost_best) / lam); a NaN cost (or a weight that is not a number)
    counts 0 and its tape is left out; no positive weight at all gives sample 0."""
    cost = cost.to(samples.dtype)
    idx = first_minimum(cost)
    best = cost.gather(0, idx.view(1, -1))[0]
    inv = 0.0 if math.isinf(lam) else 1.0 / float(lam)
    w = torch.exp(-(cost - best) * inv)
    w = torch.where(torch.isnan(w) | torch.isnan(cost), torch.zeros_like(w), w)
    wv = w.view(w.shape[0], 1, w.shape[1], 1)
    num = torch.where(wv > 0, wv * samples, torch.zeros_like(samples)).sum(0)
    W = w.sum(0).view(1, -1, 1)
    mean = torch.where(W > 0, _clamp(num / W), samples[0])
    return mean, idx


def tape_sample_max(model, horizon):
    """the most samples per env one eb_rollout_tape_sample launch takes for `model` and `horizon`"""
    limit = C.c_int32(0)
    model.api.check(model.api.sample_fn('eb_rollout_tape_sample_max')(model.handle, int(horizon), C.byref(limit)))
    return limit.value


def launch(model, obs, nominal, n_samples, seed, counter, sigma, beta, inv_lambda, ref_idx, path_id, env_ids, weights, want,
           dump_samples=False):
    """The launch behind rollout_tape_samples on prepared device tensors (obs [B, D] and nominal [H, B, 2] fp32 contiguous, ref_idx /
    env_ids int32 [B] or None) -> dict.  Nothing here synchronises with the host."""
    H, B, S = nominal.shape[0], obs.shape[0], int(n_samples)
    dev = obs.device
    out = {}
    if 'cost' in want:
        out['cost'] = torch.empty((S, B), dtype=torch.float32, device=dev)
    if 'best' in want:
        out['best_tape'] = torch.empty((H, B, 2), dtype=torch.float32, device=dev)
        out['best_cost'] = torch.empty((B,), dtype=torch.float32, device=dev)
        out['best_index'] = torch.empty((B,), dtype=torch.int32, device=dev)
    if 'mean' in want:
        out['mean_tape'] = torch.empty((H, B, 2), dtype=torch.float32, device=dev)
    if dump_samples:
        out['samples'] = torch.empty((S, H, B, 2), dtype=torch.float32, device=dev)

    def ptr(name):
        return out[name].data_ptr() if name in out and out[name].numel() else None
    sig = (C.c_float * 2)(float(sigma[0]), float(sigma[1]))
    w5 = None if weights is None else (C.c_float * 5)(*[float(v) for v in weights])
    rc = model.api.sample_fn('eb_rollout_tape_sample')(
        model.handle, B, S, H, obs.data_ptr(), nominal.data_ptr(), None if ref_idx is None else ref_idx.data_ptr(), int(path_id),
        None if env_ids is None else env_ids.data_ptr(), int(seed) & _U64, int(counter) & _U64, sig, float(beta), float(inv_lambda), w5,
        ptr('cost'), ptr('best_tape'), ptr('best_cost'), ptr('best_index'), ptr('mean_tape'), ptr('samples'), _stream(model.device))
    if rc != 0:
        model.api.check(rc)
    return out


def rollout_tape_samples(model, obses, nominal, n_samples, seed, counter, sigma, beta=0.0, lam=1.0, ref_indexes=None, path_index=None,
                         env_ids=None, weights=DEFAULT_WEIGHTS, want=('cost', 'best', 'mean'), dump_samples=False):
    """One eb_rollout_tape_sample launch from the shared rows `obses` [B, D] around `nominal` [H, B, 2] (raw actions) -> dict with
      cost [S, B]                                           ('cost' in want): eb_rollout_tape_cand's cost of every sampled tape;
      best_tape [H, B, 2], best_cost [B], best_index [B]    ('best'): the first minimum per env, a NaN never wins;
      mean_tape [H, B, 2]                                   ('mean'): the soft-min average with temperature `lam` (inf: plain average);
      samples [S, H, B, 2]                                  (dump_samples): the tapes as scored.
    sigma: two floats >= 0, the noise scale per action component; beta in [0, 1): AR(1) smoothing over the steps; (seed, counter) and
    env_ids [B] (None: the row index) key the noise; ref_indexes [B] (mode='training', None = the model's own) or path_index
    (mode='selecting', None = the model's current path).  `model`'s own state is not touched."""
    need_fp32(model, 'sample.rollout_tape_samples: fp32 state only')
    model.api.sample_fn('eb_rollout_tape_sample')          # EbError before any work when the library has no such entry
    want = tuple(want)
    for k in want:
        if k not in ('cost', 'best', 'mean'):
            raise ValueError("want: a subset of ('cost', 'best', 'mean'); got %r" % (k,))
    five_weights(weights, optional=True)
    if len(tuple(sigma)) != 2:
        raise ValueError('sigma: two floats, one per action component')
    if not lam > 0:
        raise ValueError('lam must be positive (inf: the plain average)')
    obs = check_rows(model, _dev(obses, model.device).detach().contiguous())
    B = obs.shape[0]
    nom = _dev(nominal, model.device).detach().contiguous()
    if nom.dim() != 3 or nom.shape[1] != B or nom.shape[2] != 2 or nom.shape[0] < 1:
        raise ValueError('nominal must be [H, %d, 2]; got %s' % (B, tuple(nom.shape)))
    ri, pid = path_args(model, B, ref_indexes, path_index)
    ids = None
    if env_ids is not None:
        ids = _dev(env_ids, model.device, torch.int32).contiguous()
        if tuple(ids.shape) != (B,):
            raise ValueError('env_ids must be [%d]; got %s' % (B, tuple(ids.shape)))
    inv = 0.0 if math.isinf(lam) else 1.0 / float(lam)
    return launch(model, obs, nom, n_samples, seed, counter, sigma, beta, inv, ri, pid, ids, weights, want, dump_samples)
