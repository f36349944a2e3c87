"""K candidate action tapes per env from ONE shared scene, in one launch: rollout_tape_candidates.

Everything that plans on the model asks "what do these K tapes cost from this one state?": the reference's decision loop scores one
candidate per path of the task (hier_decision.py:113-121), a line search several step lengths, a multi-start solver its starts.  The
vehicles of a scene do not depend on the ego (DAM:195, 331, 402), so eb_rollout_tape_cand (include/envbuild_cand.h,
csrc/eb_rollout_tape_cand.hip) advances a scene's vehicle records once per env and runs only the ego's chain per candidate.

    out5, cost = rollout_tape_candidates(model, obses, tapes, ref_indexes=ref)        # tapes [K, H, B, 2] -> out5 [K, H, 5, B]
    _, cost = rollout_tape_candidates(model, obses, tapes, ref_indexes=ref, weights=(-1, 10, 0, 0, 0), want_out5=False)   # [K, B]

out5[k] is bit for bit EnvironmentModel.rollout_tape's out5 for (obses, tapes[k], candidate k's path).  fp32 state only; no CPU path
and no fall-back to K separate rollouts: without the HIP library's entry this raises.

rollout_tape_candidates_grad is the same set with dJ/du of every tape (eb_rollout_tape_cand_vjp, include/envbuild_cand_grad.h):

    cost, g_tapes, _, _ = rollout_tape_candidates_grad(model, obses, tapes, (-1, 10, 0, 0, 0), ref_indexes=ref)   # [K, B], [K, H, B, 2]
"""
import ctypes as C

import torch

from ._tape_args import check_rows, five_weights, need_fp32
from .dynamics_and_models import _dev, _stream

__all__ = ['rollout_tape_candidates', 'tape_cand_max', 'rollout_tape_candidates_grad', 'tape_cand_grad_max']


def tape_cand_max(model, horizon):
    """the most candidates one eb_rollout_tape_cand launch takes for `model` (its slot count decides); larger sets go in chunks"""
    limit = C.c_int32(0)
    model.api.check(model.api.cand_fn('eb_rollout_tape_cand_max')(model.handle, int(horizon), C.byref(limit)))
    return limit.value


def _chunk_loop(fn, limit, model, obs, tapes, ref_idx, path_ids, retrack, w5, outputs):
    """fn (eb_rollout_tape_cand or eb_rollout_tape_cand_vjp) over the K candidates of tapes in chunks of `limit`; outputs: the entry's
    output tensors [K, ...] or None, in its argument order -> launches"""
    K, H, B = tapes.shape[0], tapes.shape[1], obs.shape[0]
    per_cand = ref_idx is not None and ref_idx.dim() == 2
    launches = 0
    for k0 in range(0, K, limit):
        k1 = min(K, k0 + limit)
        ri = None if ref_idx is None else (ref_idx[k0:k1] if per_cand else ref_idx)
        ids = None if path_ids is None else (C.c_int32 * (k1 - k0))(*path_ids[k0:k1])
        rc = fn(model.handle, B, k1 - k0, H, obs.data_ptr(), tapes[k0:k1].data_ptr(), None if ri is None else ri.data_ptr(),
                B if per_cand else 0, None if ids is None else C.cast(ids, C.c_void_p), 0, 1 if retrack else 0, w5,
                *[None if o is None else o[k0:k1].data_ptr() for o in outputs], _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        launches += 1
    return launches


def launch_chunks(model, obs, tapes, ref_idx, path_ids, retrack, weights, want_out5):
    """The launches behind rollout_tape_candidates on prepared device tensors: obs [B, D], tapes [K, H, B, 2], ref_idx int32 [B] or
    [K, B] (training) or None, path_ids a list of K ints (selecting) or None.  -> (out5 or None, cost or None, launches).  A set
    beyond tape_cand_max goes in chunks of the limit: candidates are independent, so the bits are those of one launch."""
    K, H, B = tapes.shape[0], tapes.shape[1], obs.shape[0]
    fn = model.api.cand_fn('eb_rollout_tape_cand')
    out5 = torch.empty((K, H, 5, B), dtype=torch.float32, device=obs.device) if want_out5 else None
    cost = torch.empty((K, B), dtype=torch.float32, device=obs.device) if weights is not None else None
    if K == 0 or B == 0:
        return out5, cost, 0
    w5 = None if weights is None else (C.c_float * 5)(*[float(v) for v in weights])
    launches = _chunk_loop(fn, tape_cand_max(model, H), model, obs, tapes, ref_idx, path_ids, retrack, w5, (out5, cost))
    return out5, cost, launches


def _prepare(model, obses, action_tapes, ref_indexes, path_indexes):
    """argument checks and path handling of both entries -> (obs [B, D], tapes [K, H, B, 2], ref_idx or None, path ids or None)"""
    obs = check_rows(model, _dev(obses, model.device).detach())
    B = obs.shape[0]
    tapes = _dev(action_tapes, model.device).detach()
    if tapes.dim() != 4 or tapes.shape[2] != B or tapes.shape[3] != 2 or tapes.shape[1] < 1:
        raise ValueError('action_tapes must be [K, H, %d, 2]; got %s' % (B, tuple(tapes.shape)))
    K = tapes.shape[0]
    ri, ids = None, None
    if model.mode == 'training':
        if ref_indexes is None:
            ri = model._path_args()[0]
        else:
            ri = _dev(ref_indexes, model.device, torch.int32)
        if tuple(ri.shape) not in ((B,), (K, B)):
            raise ValueError('ref_indexes must be [%d] or [%d, %d]; got %s' % (B, K, B, tuple(ri.shape)))
    else:
        if path_indexes is None:
            path_indexes = model._path_args()[1]
        ids = [int(path_indexes)] * K if isinstance(path_indexes, int) else [int(v) for v in path_indexes]
        if len(ids) != K:
            raise ValueError('path_indexes must be an int or %d ints; got %d' % (K, len(ids)))
    return obs, tapes, ri, ids


def rollout_tape_candidates(model, obses, action_tapes, ref_indexes=None, path_indexes=None, retrack=False, weights=None,
                            want_out5=True):
    """Value-only open-loop rollout of K tapes per env from the shared rows `obses` [B, D]: action_tapes [K, H, B, 2] raw ->
    (out5 [K, H, 5, B] or None, cost [K, B] or None).
      ref_indexes   mode='training': [B] (every candidate on the env's path) or [K, B]; None = the model's own (reset);
      path_indexes  mode='selecting': an int (all candidates) or K ints; None = the model's current path;
      retrack       True: every (env, candidate) starts from the tracking error of the row's own pose on the CANDIDATE's path instead
                    of obses' columns 6-8 (the reference builds one obs per path, hier_decision.py:113-117);
      weights       five floats: cost[k] = sum_t w . out5[k][t] in the order include/envbuild_cand.h fixes; None = no cost;
      want_out5     False: the cost only.
    `model` (an EnvironmentModel with fp32 state) supplies the task, the slot modes and the tables; its own state is not touched."""
    need_fp32(model, 'cand.rollout_tape_candidates: fp32 state only (the fp16-state kernels have no candidate form)')
    model.api.cand_fn('eb_rollout_tape_cand')              # EbError before any work when the library has no such entry
    if weights is None and not want_out5:
        raise ValueError('rollout_tape_candidates: nothing asked for (weights is None and want_out5 is False)')
    five_weights(weights, optional=True)
    obs, tapes, ri, ids = _prepare(model, obses, action_tapes, ref_indexes, path_indexes)
    out5, cost, _ = launch_chunks(model, obs, tapes, ri, ids, retrack, weights, want_out5)
    return out5, cost


def tape_cand_grad_max(model, horizon):
    """the most candidates one eb_rollout_tape_cand_vjp launch takes for `model` and `horizon` (queue and LDS tape per (env, candidate)
    decide); 0 when the horizon leaves room for none"""
    limit = C.c_int32(0)
    model.api.check(model.api.cand_grad_fn('eb_rollout_tape_cand_vjp_max')(model.handle, int(horizon), C.byref(limit)))
    return limit.value


def launch_grad_chunks(model, obs, tapes, ref_idx, path_ids, retrack, weights, want_out5, want_g_obs):
    """launch_chunks' twin for eb_rollout_tape_cand_vjp, on prepared device tensors (tapes contiguous)
    -> (cost [K, B], g_tapes [K, H, B, 2], out5 or None, g_obs0 [K, B, nd] or None, launches).  A set beyond tape_cand_grad_max goes
    in chunks of the limit: ceil(K / limit) launches, the bits of the chunks' own launches (candidates are independent)."""
    K, H, B = tapes.shape[0], tapes.shape[1], obs.shape[0]
    fn = model.api.cand_grad_fn('eb_rollout_tape_cand_vjp')
    nd = model.obs_dim - 4 * model.veh_num
    cost = torch.empty((K, B), dtype=torch.float32, device=obs.device)
    g = torch.empty((K, H, B, 2), dtype=torch.float32, device=obs.device)
    out5 = torch.empty((K, H, 5, B), dtype=torch.float32, device=obs.device) if want_out5 else None
    g_obs = torch.empty((K, B, nd), dtype=torch.float32, device=obs.device) if want_g_obs else None
    if K == 0 or B == 0:
        return cost, g, out5, g_obs, 0
    limit = tape_cand_grad_max(model, H)
    if limit < 1:
        raise ValueError('eb_rollout_tape_cand_vjp: a horizon of %d steps leaves room for no candidate on this model '
                         '(eb_rollout_tape_cand_vjp_max)' % H)
    w5 = (C.c_float * 5)(*[float(v) for v in weights])
    launches = _chunk_loop(fn, limit, model, obs, tapes, ref_idx, path_ids, retrack, w5, (out5, cost, g_obs, g))
    return cost, g, out5, g_obs, launches


def rollout_tape_candidates_grad(model, obses, action_tapes, weights, ref_indexes=None, path_indexes=None, retrack=False,
                                 want_out5=False, want_g_obs=False):
    """Cost and gradient of K tapes per env from the shared rows `obses` [B, D]: action_tapes [K, H, B, 2] raw ->
    (cost [K, B], g_tapes [K, H, B, 2], out5 [K, H, 5, B] or None, g_obs0 [K, B, nd] or None).
      weights       five floats, required: cost[k] = sum_t w . out5[k][t] (the order include/envbuild_cand.h fixes); g_tapes[k] is
                    d cost[k] / d action_tapes[k], bit for bit eb_rollout_tape_vjp's for that tape alone;
      ref_indexes, path_indexes, retrack   as rollout_tape_candidates;
      want_g_obs    the cotangent of every candidate's private copy of the row's first nd columns (after the retrack replacement).
    fp32 state only; no CPU path and no fall-back to K separate launches."""
    need_fp32(model, 'cand.rollout_tape_candidates_grad: fp32 state only (the reverse pass has no fp16-state form)')
    model.api.cand_grad_fn('eb_rollout_tape_cand_vjp')     # EbError before any work when the library has no such entry
    five_weights(() if weights is None else weights)
    obs, tapes, ri, ids = _prepare(model, obses, action_tapes, ref_indexes, path_indexes)
    cost, g, out5, g_obs, _ = launch_grad_chunks(model, obs, tapes, ri, ids, retrack, weights, want_out5, want_g_obs)
    return cost, g, out5, g_obs
