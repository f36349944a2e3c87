"""The PPO update's arithmetic on the GPU (include/envbuild_ppo.h, env_build_amd/csrc/eb_ppo.hip): generalised advantage estimation
over [T, B] arrays in ONE launch, and the clipped surrogate — ratio, clamp, minimum, entropy bonus and the cotangent of the logits — in
ONE launch with the policy network.  It is what examples/ppo_env_loop.py does in torch between `log_prob` and `backward`, and in its
reverse loop over the steps.

`gae(rewards, values, v_last, nonterminal, gamma, lam, next_values=None, carry=None)` -> (adv, ret): eb_gae.
`surrogate(net, obs, actions, logp_old, adv, action_range, clip, ...)` is the inference and diagnostics surface: the fused entry where
eb_ppo_surrogate_supported says yes (an fp32 `MLPNet`), otherwise the policy's own forward followed by eb_ppo_surrogate_from_logits —
`policy_logp.log_prob_actions`' routing.
`policy_loss(net, obs, actions, logp_old, adv, action_range, clip, ...)` is the training surface: one torch.autograd.Function on a
`TrainableMLPNet`.  Its forward is the fused launch with scale = 1 / n, which also writes the cotangent of the logits; its backward is
at most one multiply of that by the incoming scalar and one eb_mlp_backward(head = 0).
`surrogate_from_logits` wraps the elementwise entry.

`ppo_reference` and `gae_reference` restate the header's contract in NumPy; in float32 every operation is the kernels', on
`policy_logp_reference` and `policy_sample`'s single-rounding exp_det: their bits.

The entries are bound here, on `hip_api().lib`, on first use (PPO_PROTOTYPES): _capi's tables stay as they are.  There is no CPU path.
"""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi
from .dynamics_and_models import DevArray, _dev, _stream, _unwrap
from .policy import MLPNet
from .policy_logp import _actions, _logits, policy_logp_reference
from .policy_sample import _exp_det, _range

__all__ = ['gae', 'surrogate', 'surrogate_from_logits', 'policy_loss', 'ppo_reference', 'gae_reference', 'EbPpoArgs', 'EbGaeArgs',
           'EB_PPO_ABI_VERSION', 'PPO_PROTOTYPES']

_P, _I, _F = C.c_void_p, C.c_int32, C.c_float


class EbPpoArgs(C.Structure):
    """eb_ppo_args of include/envbuild_ppo.h"""
    _fields_ = [('n', _I), ('out_dim', _I), ('obs', _P), ('logits', _P), ('actions', _P), ('logp_old', _P), ('adv', _P), ('adv_norm', _P),
                ('action_range', _F), ('clip', _F), ('ent_coef', _F), ('scale', _F), ('logp', _P), ('ratio', _P), ('surr', _P), ('ent', _P),
                ('g_logits', _P), ('logits_out', _P), ('z_out', _P), ('stream', _P)]


class EbGaeArgs(C.Structure):
    """eb_gae_args of include/envbuild_ppo.h"""
    _fields_ = [('T', _I), ('n', _I), ('rewards', _P), ('values', _P), ('v_last', _P), ('nonterminal', _P), ('next_values', _P),
                ('carry', _P), ('gamma', C.c_double), ('lam', C.c_double), ('adv', _P), ('ret', _P), ('stream', _P)]


# include/envbuild_ppo.h: name -> (restype, argtypes) for every symbol the header declares
EB_PPO_ABI_VERSION = 1
HEADER = 'envbuild_ppo.h'
PPO_PROTOTYPES = {
    'eb_ppo_abi_version': (C.c_int, []),
    'eb_ppo_surrogate_supported': (C.c_int, [_P, C.POINTER(_I)]),
    'eb_ppo_surrogate': (C.c_int, [_P, C.POINTER(EbPpoArgs)]),
    'eb_ppo_surrogate_from_logits': (C.c_int, [C.POINTER(EbPpoArgs)]),
    'eb_gae': (C.c_int, [C.POINTER(EbGaeArgs)]),
}


def bind(api):
    """name -> raw ctypes function for every entry of PPO_PROTOTYPES on `api` (a _capi.CApi), bound on first use; EbError when the
    library does not export them or speaks another version."""
    fns = api.__dict__.setdefault('_ppo_fns', {})
    if not fns:
        missing = [n for n in PPO_PROTOTYPES if not hasattr(api.lib, n)]
        if missing:
            raise _capi.EbError('%s (backend %r) does not export %s: this library has no PPO surrogate or advantage estimation (include/%s '
                                'is implemented by the HIP library only; rebuild an older one)' % (api.path, api.backend, ', '.join(missing), HEADER))
        for n, (res, args) in PPO_PROTOTYPES.items():
            fn = getattr(api.lib, n)
            fn.restype, fn.argtypes = res, args
            fns[n] = fn
        v = fns['eb_ppo_abi_version']()
        if v != EB_PPO_ABI_VERSION:
            fns.clear()
            raise _capi.EbError('%s: ppo ABI version %d, expected %d (include/%s)' % (api.path, v, EB_PPO_ABI_VERSION, HEADER))
    return fns


def _call(api, name, *args):
    api.check(bind(api)[name](*args))


def _args(stream, n, out_dim=0, action_range=0.0, clip=0.0, ent_coef=0.0, scale=1.0, **tensors):
    """eb_ppo_args: the named fields from device tensors (None: NULL), the rest NULL"""
    a = EbPpoArgs(n=n, out_dim=out_dim, action_range=action_range, clip=clip, ent_coef=ent_coef, scale=scale, stream=stream)
    for k, t in tensors.items():
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def _gae_args(stream, T, n, gamma, lam, **tensors):
    """eb_gae_args: the named fields from device tensors (None: NULL), the rest NULL"""
    a = EbGaeArgs(T=T, n=n, gamma=gamma, lam=lam, stream=stream)
    for k, t in tensors.items():
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def _scalar(x, name, lowest=None):
    x = float(x)
    if x != x or (lowest is not None and x < lowest):
        raise ValueError('%s must be a number%s, got %r' % (name, '' if lowest is None else ' >= %g' % lowest, x))
    return x


# ---- generalised advantage estimation -------------------------------------------------------------------------------------------------
def gae(rewards, values, v_last, nonterminal, gamma, lam, next_values=None, carry=None):
    """eb_gae: advantages and returns of [T, B] rewards, values and nonterminal flags (floats: 0 where the step ended its episode) and
    the value [B] after the last step -> (adv [T, B], ret [T, B] = adv + values) as DevArrays.  One launch.

    With next_values and carry None it is the reverse loop of examples/ppo_env_loop.py bit for bit.  next_values [T, B] replaces the
    next step's value as the bootstrap of every step (v_last is then not read and may be None); carry [T, B] replaces nonterminal as the
    factor of the running advantage: a time-limit truncation is nonterminal = 1, carry = 0 and next_values = the value of the final
    observation at that step."""
    r = _unwrap(rewards)
    if not (isinstance(r, torch.Tensor) and r.is_cuda):
        raise TypeError('rewards must live on the GPU (a DevArray or a device tensor): there is no CPU path')
    r = r.detach().to(dtype=torch.float32).contiguous()
    if r.dim() != 2 or r.shape[0] < 1 or r.shape[0] > 65535:
        raise ValueError('rewards must be [T, B] with T in 1..65535, got %s' % (tuple(r.shape),))
    T, n = r.shape
    g, l = float(gamma), float(lam)
    if not (math.isfinite(g) and math.isfinite(l)):
        raise ValueError('gamma and lam must be finite, got %r and %r' % (gamma, lam))

    def arr(x, name, shape):
        if x is None:
            return None
        x = _unwrap(x)
        t = _dev(x.detach() if isinstance(x, torch.Tensor) else x, r.device)
        if tuple(t.shape) != shape:
            raise ValueError('%s must be %s, got %s' % (name, list(shape), tuple(t.shape)))
        return t
    v, live = arr(values, 'values', (T, n)), arr(nonterminal, 'nonterminal', (T, n))
    nv, cy = arr(next_values, 'next_values', (T, n)), arr(carry, 'carry', (T, n))
    vl = arr(v_last, 'v_last', (n,))
    if v is None or live is None or (vl is None and nv is None):
        raise ValueError('values and nonterminal are required, and v_last unless next_values is given')
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    with torch.cuda.device(r.device):
        _call(_capi.hip_api(), 'eb_gae', C.byref(_gae_args(_stream(r.device), T, n, g, l, rewards=r, values=v, v_last=vl, nonterminal=live,
                                                            next_values=nv, carry=cy, adv=adv, ret=ret)))
    return DevArray(adv), DevArray(ret)


# ---- the surrogate: inference and diagnostics ---------------------------------------------------------------------------------------------
_WANT = ('ratio', 'surr', 'ent', 'g_logits', 'logits', 'z')
_FIELD = {'logits': 'logits_out', 'z': 'z_out'}


def _outputs(want, n, out_dim, device):
    unknown = [w for w in want if w not in _WANT]
    if unknown:
        raise ValueError('want: unknown output %r (of %r)' % (unknown[0], _WANT))
    shapes = {'logp': (n,), 'ratio': (n,), 'surr': (n,), 'ent': (n,), 'g_logits': (n, out_dim), 'logits': (n, out_dim), 'z': (n, out_dim // 2)}
    return {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in ('logp',) + tuple(w for w in _WANT if w in want)}


def _rows(n, device, logp_old, adv, adv_norm):
    """the per-row inputs on the device: logp_old [n], adv [n], adv_norm [2] or None"""
    lo, ad = _dev(_detached(logp_old), device), _dev(_detached(adv), device)
    if tuple(lo.shape) != (n,) or tuple(ad.shape) != (n,):
        raise ValueError('logp_old and adv must be [%d], got %s and %s' % (n, tuple(lo.shape), tuple(ad.shape)))
    an = None
    if adv_norm is not None:
        an = _dev(_detached(adv_norm), device)
        if tuple(an.shape) != (2,):
            raise ValueError('adv_norm must hold two floats (mean, 1 / std), got %s' % (tuple(an.shape),))
    return lo, ad, an


def _detached(x):
    x = _unwrap(x)
    return x.detach() if isinstance(x, torch.Tensor) else x


def _out_fields(out):
    return {_FIELD.get(k, k): v for k, v in out.items()}


def surrogate_from_logits(logits, actions, logp_old, adv, action_range, clip, ent_coef=0.0, adv_norm=None, want=(), scale=None):
    """eb_ppo_surrogate_from_logits: the surrogate row alone on [B, 2 * act_dim] logits -> {'logp': [B], ...} as DevArrays ('logp' and
    what `want` names of 'ratio', 'surr', 'ent', 'g_logits', 'z'; 'logits' hands back the input).  scale None: 1 / B."""
    t = _logits(logits)
    n, out_dim = t.shape
    a = _actions(actions, n, out_dim // 2, t.device)
    lo, ad, an = _rows(n, t.device, logp_old, adv, adv_norm)
    out = _outputs([w for w in want if w != 'logits'], n, out_dim, t.device)
    sc = 1.0 / max(n, 1) if scale is None else _scalar(scale, 'scale')
    with torch.cuda.device(t.device):
        _call(_capi.hip_api(), 'eb_ppo_surrogate_from_logits',
              C.byref(_args(_stream(t.device), n, out_dim, _range(action_range), _scalar(clip, 'clip', 0.0), _scalar(ent_coef, 'ent_coef'), sc,
                            logits=t, actions=a, logp_old=lo, adv=ad, adv_norm=an, **_out_fields(out))))
    if 'logits' in want:
        out['logits'] = t
    return {k: DevArray(v) for k, v in out.items()}


def _supported(net):
    ok = C.c_int32(0)
    _call(net.api, 'eb_ppo_surrogate_supported', net._handle, C.byref(ok))
    return bool(ok.value)


def _fused(net, x, a, lo, ad, an, ar, clip, ent_coef, scale, out):
    _call(net.api, 'eb_ppo_surrogate', net._handle,
          C.byref(_args(net._stream(), x.shape[0], 0, ar, clip, ent_coef, scale, obs=x, actions=a, logp_old=lo, adv=ad, adv_norm=an,
                        **_out_fields(out))))


def surrogate(net, obs, actions, logp_old, adv, action_range, clip, ent_coef=0.0, adv_norm=None, want=(), scale=None):
    """The clipped surrogate of the policy `net` at obs [B, obs_dim] for stored actions [B, act_dim], their logp_old [B] and advantages
    adv [B] -> {'logp': [B], ...} as DevArrays: 'logp' and what `want` names of 'ratio', 'surr' (unscaled), 'ent' (unscaled), 'g_logits'
    (the cotangent of the logits for -scale * sum(surr) - scale * ent_coef * sum(ent)), 'logits' and 'z'.

    adv_norm: two floats on the device, (mean, 1 / std), applied to adv in the kernel; None: adv as it is.  scale None: 1 / B.
    An fp32 `MLPNet` (a `TrainableMLPNet` included) takes the fused entry, one launch; any other policy — an fp16 `MLPNet`, a callable
    that returns logits — its own forward followed by eb_ppo_surrogate_from_logits.  Same numbers either way on an fp32 handle."""
    ar = _range(action_range)
    if isinstance(net, MLPNet):
        if net.output_dim < 2 or net.output_dim % 2:
            raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
        if _supported(net):
            x = net._in(_detached(obs))
            n = x.shape[0]
            out = _outputs(want, n, net.output_dim, net.device)
            lo, ad, an = _rows(n, net.device, logp_old, adv, adv_norm)
            sc = 1.0 / max(n, 1) if scale is None else _scalar(scale, 'scale')
            _fused(net, x, _actions(actions, n, net.output_dim // 2, net.device), lo, ad, an, ar, _scalar(clip, 'clip', 0.0),
                   _scalar(ent_coef, 'ent_coef'), sc, out)
            return {k: DevArray(v) for k, v in out.items()}
        logits = MLPNet.call(net, obs)
    else:
        logits = net(obs)
    return surrogate_from_logits(logits, actions, logp_old, adv, action_range, clip, ent_coef, adv_norm, want, scale)


# ---- the surrogate: training ------------------------------------------------------------------------------------------------------------------
class _PolicyLoss(torch.autograd.Function):
    """the PPO policy loss of a TrainableMLPNet: forward the fused launch (g_logits written there) and two reductions, backward
    eb_mlp_backward(head = 0) alone"""

    @staticmethod
    def forward(ctx, net, consts, actions, lo, ad, an, x, *params):
        ar, clip, ent_coef = consts
        ent_coef = float(np.float32(ent_coef))             # the number the entry's float field holds: loss and g_logits share it
        net._sync()
        n = x.shape[0]
        out = _outputs(('ratio', 'surr', 'ent', 'g_logits'), n, net.output_dim, net.device)
        _fused(net, x, actions, lo, ad, an, ar, clip, ent_coef, 1.0 / n, out)
        ctx.net, ctx.version = net, net._flat._version
        ctx.save_for_backward(x, out['g_logits'])
        # the two reductions accumulate in float64 and the result is rounded once: the loss is then as good as its rows
        loss = (-(out['surr'].sum(dtype=torch.float64) + ent_coef * out['ent'].sum(dtype=torch.float64)) / n).to(torch.float32)
        rows = (out['logp'], out['ratio'], out['surr'], out['ent'])
        ctx.mark_non_differentiable(*rows)
        return (loss,) + rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, *_rows):
        net, (x, g_logits) = ctx.net, ctx.saved_tensors
        if net._flat._version != ctx.version:
            raise RuntimeError('the weights of %s were modified in place between this forward and its backward (version %d, expected %d): '
                               'the gradient would be that of another network' % (net.name, net._flat._version, ctx.version))
        n_in = 7
        net._sync()
        n = x.shape[0]
        g_out = g_logits * g_loss.to(dtype=torch.float32)          # the one torch launch; the stored cotangent stays as the forward wrote it
        need = C.c_size_t(0)
        net.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=net.device)
        g_obs = torch.empty_like(x) if ctx.needs_input_grad[n_in - 1] else None
        g_flat = torch.empty_like(net._flat) if any(ctx.needs_input_grad[n_in:]) else None
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        net.api.mlp_backward(net._h, n, p(x), p(g_out), 0, C.c_float(0.0), p(ws), need.value, None, p(g_obs), p(g_flat), net._stream())
        grads = [None] * len(net._params) if g_flat is None else [g_flat[a:b].view(shape) for a, b, shape in net._slices]
        return (None,) * (n_in - 1) + (g_obs,) + tuple(grads)


def policy_loss(net, obs, actions, logp_old, adv, action_range, clip, ent_coef=0.0, adv_norm=None):
    """(loss, rows): the PPO policy loss -mean(surr) - ent_coef * mean(ent) of the TrainableMLPNet `net` as a 0-dim tensor on the autograd
    graph — one node — and a dict of detached per-row tensors 'logp', 'ratio', 'surr', 'ent' [B] for logging (clip fraction, approximate
    KL).  The gradient reaches obs, when it requires grad, and every parameter of the network; none goes to the actions, logp_old or the
    advantages.  Forward is one launch and two torch means; backward is one multiply by the incoming scalar and one eb_mlp_backward."""
    from .policy_grad import TrainableMLPNet
    if not isinstance(net, TrainableMLPNet):
        raise TypeError('policy_loss differentiates a TrainableMLPNet, got %s (surrogate serves inference)' % type(net).__name__)
    if net.output_dim < 2 or net.output_dim % 2:
        raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
    x = net._graph_in(obs)
    if not _supported(net):
        net.api.check(-1)                                    # the C reason: an fp16 handle has no gradient
    n = x.shape[0]
    if n < 1:
        raise ValueError('policy_loss needs at least one row')
    a = _actions(actions, n, net.output_dim // 2, net.device)
    lo, ad, an = _rows(n, net.device, logp_old, adv, adv_norm)
    consts = (_range(action_range), _scalar(clip, 'clip', 0.0), _scalar(ent_coef, 'ent_coef'))
    loss, logp, ratio, surr, ent = _PolicyLoss.apply(net, consts, a, lo, ad, an, x, *net._params)
    return loss, dict(logp=logp, ratio=ratio, surr=surr, ent=ent)


# ---- the contract in NumPy ----------------------------------------------------------------------------------------------------------
_f = np.float32


def ppo_reference(logits, actions, logp_old, adv, action_range, clip, ent_coef=0.0, scale=None, adv_norm=None, dtype=np.float32):
    """The surrogate row of include/envbuild_ppo.h in NumPy -> dict(logp, z, A, ratio, surr, ent, g_lp, g_logits, loss).

    logits [n, 2 * act_dim]: the activated outputs of the network; adv_norm: (mean, 1 / std) or None; scale None: 1 / n.
    loss = -scale * sum(surr) - scale * ent_coef * sum(ent), accumulated in float64 (the kernels do not form it).
    dtype float32: the kernels' operations one by one on policy_logp_reference and exp_det — their bits.  dtype float64: the same formulas
    with the library exponential — the yardstick."""
    dtype = np.dtype(dtype).type
    f32 = dtype == np.float32
    logp, z, _ = policy_logp_reference(logits, actions, action_range, dtype=dtype)
    y = np.asarray(logits).astype(dtype)
    n, act_dim = y.shape[0], y.shape[1] // 2
    ls = y[:, act_dim:]
    sc = dtype(1.0 / max(n, 1) if scale is None else scale)
    cl, ec = dtype(clip), dtype(ent_coef)
    lo, hi = dtype(1) - cl, dtype(1) + cl
    w, g_ent = -sc, -(sc * ec)
    with np.errstate(all='ignore'):
        A = np.asarray(adv).astype(dtype)
        if adv_norm is not None:
            an = np.asarray(adv_norm).astype(dtype)
            A = (A - an[0]) * an[1]
        d = logp - np.asarray(logp_old).astype(dtype)
        r = _exp_det(d) if f32 else np.exp(d)
        s1 = r * A
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
        s2 = rc * A
        surr = np.where(s2 < s1, s2, s1)
        ent = np.zeros(n, dtype)
        for k in range(act_dim):
            ent = ent + ls[:, k]
        ent = ent + dtype(act_dim) * dtype(_f(1.4189385332) if f32 else 0.5 * math.log(2.0 * math.pi * math.e))
        blocked = ((r < lo) | (r > hi)) & (s2 <= s1)
        g_lp = np.where(blocked, dtype(0), (w * A) * r).astype(dtype)
        inv = _exp_det(-ls) if f32 else np.exp(-ls)
        g_lp2 = g_lp.reshape(-1, 1)
        g_y = np.concatenate([g_lp2 * (z * inv), g_lp2 * (z * z - dtype(1)) + g_ent], axis=1).astype(dtype)
        loss = -float(sc) * float(np.sum(surr, dtype=np.float64)) - float(sc) * float(ec) * float(np.sum(ent, dtype=np.float64))
    return dict(logp=logp, z=z, A=A.astype(dtype), ratio=r.astype(dtype), surr=surr.astype(dtype), ent=ent.astype(dtype), g_lp=g_lp,
                g_logits=g_y, loss=loss)


def gae_reference(rewards, values, v_last, nonterminal, gamma, lam, next_values=None, carry=None, dtype=np.float32):
    """eb_gae's contract in NumPy on [T, n] arrays -> (adv, ret).  dtype float32: the kernel's operations in its order, gamma as a float
    and gl = float32(gamma * lam): its bits.  dtype float64: the same recursion in double."""
    dtype = np.dtype(dtype).type
    rw, v, live = (np.asarray(x).astype(dtype) for x in (rewards, values, nonterminal))
    cy = live if carry is None else np.asarray(carry).astype(dtype)
    nv = None if next_values is None else np.asarray(next_values).astype(dtype)
    T, n = rw.shape
    g, gl = dtype(gamma), dtype(float(gamma) * float(lam))
    adv = np.empty((T, n), dtype)
    run = np.zeros(n, dtype)
    with np.errstate(all='ignore'):
        for t in range(T - 1, -1, -1):
            vn = nv[t] if nv is not None else (np.asarray(v_last).astype(dtype) if t == T - 1 else v[t + 1])
            delta = (rw[t] + (g * vn) * live[t]) - v[t]
            run = delta + (gl * cy[t]) * run
            adv[t] = run
        ret = adv + v
    return adv, ret
