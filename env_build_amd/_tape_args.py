"""The argument checks the tape entries' Python callers share (mpc.py, cand.py, sample.py, ilqr.py, grad.py): one text per refusal."""
import torch

from . import _capi
from .dynamics_and_models import _dev


def need_fp32(model, message):
    """the tape kernels are fp32-state only: EbError(message) for any other model"""
    if model.state_dtype != torch.float32:
        raise _capi.EbError(message)


def check_rows(model, obs):
    """obs, if it is [B, obs_dim] rows of `model`"""
    if obs.dim() != 2 or obs.shape[1] != model.obs_dim:
        raise ValueError('obses must be [B, %d]; got %s' % (model.obs_dim, tuple(obs.shape)))
    return obs


def five_weights(weights, optional=False):
    """the weights of a cost as a tuple of five floats, one per out5 row (optional: None stays None)"""
    if weights is None and optional:
        return None
    w = tuple(float(v) for v in weights)
    if len(w) != 5:
        raise ValueError('weights: five floats, one per out5 row')
    return w


def tapes_or_zeros(model, tapes, shape, what):
    """`tapes` on the model's device if it has exactly `shape`; None = the zero tapes of that shape"""
    if tapes is None:
        return torch.zeros(shape, dtype=torch.float32, device=model.device)
    t = _dev(tapes, model.device).detach()
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be [%s]; got %s' % (what, ', '.join(str(v) for v in shape), tuple(t.shape)))
    return t


def path_args(model, B, ref_indexes, path_index):
    """The path of a one-path launch -> (ref_idx int32 [B] on the device or None, path id): mode='training' reads ref_indexes (None =
    the model's own), mode='selecting' path_index (None = the model's current path)."""
    if model.mode != 'training':
        return None, int(model._path_args()[1] if path_index is None else path_index)
    ri = model._path_args()[0] if ref_indexes is None else _dev(ref_indexes, model.device, torch.int32)
    if ri is not None and tuple(ri.shape) != (B,):
        raise ValueError('ref_indexes must be [%d]; got %s' % (B, tuple(ri.shape)))
    return ri, 0
