"""The log-probability of GIVEN actions under the policy on the GPU (include/envbuild_policy_logp.h, env_build_amd/csrc/eb_policy_logp.hip):
what a trainer does with the distribution the reference's Policy4Toyota._logits2dist returns (utils/policy.py:71-82) — log_prob of
actions it stored earlier, old samples under new weights: likelihood ratios (PPO, off-policy corrections) and maximum-likelihood
fitting of the policy to given actions.  `policy_sample` returns the log-probability of its own draw only, and differentiates with the
noise fixed; here the action is data and the derivatives go to the mean and the log-std.

`log_prob_actions(net, obs, actions, action_range, want=())` is the inference surface: network and epilogue in ONE launch where
eb_policy_logp_supported says yes (an fp32 `MLPNet`), otherwise `net(obs)` followed by eb_policy_logp_from_logits (an fp16 `MLPNet`, any
callable policy that returns [B, 2 * act_dim] logits).
`log_prob(net, obs, actions, action_range)` is the training surface: one torch.autograd.Function on a `TrainableMLPNet` that returns
(logp, logits), BOTH on the graph; its backward is eb_policy_logp_vjp, plus the cotangent that arrived for the logits (an entropy bonus,
a KL to stored logits), then one eb_mlp_backward(head = 0), with gradients to obs and to every parameter and none to the actions.
`log_prob_from_logits` / `log_prob_vjp` wrap the two elementwise entries.

`policy_logp_reference` restates the header's contract in NumPy; in float32 every operation is the kernels', on `policy_sample`'s
single-rounding fmaf, exp_det and log_det: their bits.

The entries are bound here, on `hip_api().lib`, on first use (POLICY_LOGP_PROTOTYPES): _capi's tables stay as they are.  There is no CPU
path.
"""
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi
from .dynamics_and_models import DevArray, _dev, _stream, _unwrap
from .policy import MLPNet
from .policy_sample import _exp_det, _log_det, _range

__all__ = ['log_prob_actions', 'log_prob_from_logits', 'log_prob_vjp', 'log_prob', 'policy_logp_reference', 'EbPolicyLogpArgs',
           'EB_POLICY_LOGP_ABI_VERSION', 'POLICY_LOGP_PROTOTYPES']

_P, _I, _F = C.c_void_p, C.c_int32, C.c_float


class EbPolicyLogpArgs(C.Structure):
    """eb_policy_logp_args of include/envbuild_policy_logp.h"""
    _fields_ = [('n', _I), ('out_dim', _I), ('obs', _P), ('logits', _P), ('actions', _P), ('action_range', _F), ('logp', _P),
                ('logits_out', _P), ('z_out', _P), ('z', _P), ('g_logp', _P), ('g_logits', _P), ('stream', _P)]


# include/envbuild_policy_logp.h: name -> (restype, argtypes) for every symbol the header declares
EB_POLICY_LOGP_ABI_VERSION = 1
HEADER = 'envbuild_policy_logp.h'
POLICY_LOGP_PROTOTYPES = {
    'eb_policy_logp_abi_version': (C.c_int, []),
    'eb_policy_logp_supported': (C.c_int, [_P, C.POINTER(_I)]),
    'eb_policy_logp': (C.c_int, [_P, C.POINTER(EbPolicyLogpArgs)]),
    'eb_policy_logp_from_logits': (C.c_int, [C.POINTER(EbPolicyLogpArgs)]),
    'eb_policy_logp_vjp': (C.c_int, [C.POINTER(EbPolicyLogpArgs)]),
}


def bind(api):
    """name -> raw ctypes function for every entry of POLICY_LOGP_PROTOTYPES on `api` (a _capi.CApi), bound on first use; EbError when
    the library does not export them or speaks another version."""
    fns = api.__dict__.setdefault('_policy_logp_fns', {})
    if not fns:
        missing = [n for n in POLICY_LOGP_PROTOTYPES if not hasattr(api.lib, n)]
        if missing:
            raise _capi.EbError('%s (backend %r) does not export %s: this library has no log-probability of given actions (include/%s is '
                                'implemented by the HIP library only; rebuild an older one)' % (api.path, api.backend, ', '.join(missing), HEADER))
        for n, (res, args) in POLICY_LOGP_PROTOTYPES.items():
            fn = getattr(api.lib, n)
            fn.restype, fn.argtypes = res, args
            fns[n] = fn
        v = fns['eb_policy_logp_abi_version']()
        if v != EB_POLICY_LOGP_ABI_VERSION:
            fns.clear()
            raise _capi.EbError('%s: policy-logp ABI version %d, expected %d (include/%s)' % (api.path, v, EB_POLICY_LOGP_ABI_VERSION, HEADER))
    return fns


def _call(api, name, *args):
    api.check(bind(api)[name](*args))


def _args(stream, n, out_dim=0, action_range=0.0, **tensors):
    """the argument struct: the named fields from device tensors (None: NULL), the rest NULL"""
    a = EbPolicyLogpArgs(n=n, out_dim=out_dim, action_range=action_range, stream=stream)
    for k, t in tensors.items():
        setattr(a, k, None if t is None else t.data_ptr())
    return a


def _logits(logits):
    t = _unwrap(logits)
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError('logits must live on the GPU (a DevArray or a device tensor): there is no CPU path')
    t = t.detach().to(dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] < 2 or t.shape[1] % 2 or t.shape[1] > 32:
        raise ValueError('logits must be [B, 2 * act_dim] with act_dim in 1..16, got %s' % (tuple(t.shape),))
    return t


def _actions(actions, n, act_dim, device):
    a = _unwrap(actions)
    a = _dev(a.detach() if isinstance(a, torch.Tensor) else a, device)
    if tuple(a.shape) != (n, act_dim):
        raise ValueError('actions must be [%d, %d], got %s' % (n, act_dim, tuple(a.shape)))
    return a


_WANT = ('logits', 'z')


def _outputs(want, n, out_dim, device):
    unknown = [w for w in want if w not in _WANT]
    if unknown:
        raise ValueError('want: unknown output %r (of %r)' % (unknown[0], _WANT))
    shapes = {'logp': (n,), 'logits': (n, out_dim), 'z': (n, out_dim // 2)}
    return {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in ('logp',) + tuple(w for w in _WANT if w in want)}


def log_prob_from_logits(logits, actions, action_range, want=()):
    """eb_policy_logp_from_logits: the epilogue alone on [B, 2 * act_dim] logits (what `MLPNet.call` returns) and actions [B, act_dim]
    -> {'logp': [B], 'z': [B, act_dim]} as DevArrays ('logp' and what `want` names; 'logits' hands back the input)."""
    t = _logits(logits)
    n, out_dim = t.shape
    a = _actions(actions, n, out_dim // 2, t.device)
    out = _outputs([w for w in want if w != 'logits'], n, out_dim, t.device)
    with torch.cuda.device(t.device):
        _call(_capi.hip_api(), 'eb_policy_logp_from_logits',
              C.byref(_args(_stream(t.device), n, out_dim, _range(action_range), logits=t, actions=a, logp=out['logp'], z_out=out.get('z'))))
    if 'logits' in want:
        out['logits'] = t
    return {k: DevArray(v) for k, v in out.items()}


def log_prob_vjp(logits, z, g_logp):
    """eb_policy_logp_vjp: the cotangent of the logits [B, 2 * act_dim] from that of logp [B] and the z [B, act_dim] the forward wrote
    -> DevArray.  The actions are data: nothing else is read."""
    t = _logits(logits)
    n, out_dim = t.shape
    zz, gl = _dev(z, t.device), _dev(g_logp, t.device)
    if tuple(zz.shape) != (n, out_dim // 2) or tuple(gl.shape) != (n,):
        raise ValueError('z must be [%d, %d] and g_logp [%d]' % (n, out_dim // 2, n))
    g = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _call(_capi.hip_api(), 'eb_policy_logp_vjp', C.byref(_args(_stream(t.device), n, out_dim, logits=t, z=zz, g_logp=gl, g_logits=g)))
    return DevArray(g)


def _supported(net):
    ok = C.c_int32(0)
    _call(net.api, 'eb_policy_logp_supported', net._handle, C.byref(ok))
    return bool(ok.value)


def _fused(net, x, a, ar, out):
    _call(net.api, 'eb_policy_logp', net._handle,
          C.byref(_args(net._stream(), x.shape[0], 0, ar, obs=x, actions=a, logp=out['logp'], logits_out=out.get('logits'), z_out=out.get('z'))))


def log_prob_actions(net, obs, actions, action_range, want=()):
    """log pi(actions | obs) [B] of the policy `net` at obs [B, obs_dim] for GIVEN actions [B, act_dim], with what `want` names of
    'logits' ([B, 2 * act_dim]) and 'z' (the standardised pre-squash value, [B, act_dim]) -> {'logp': ..., ...} as DevArrays.

    action_range None: no squashing.  An action at or beyond +-action_range is taken just inside it (the header's clamp): finite.
    An fp32 `MLPNet` (a `TrainableMLPNet` included) takes the fused entry, one launch; any other policy — an fp16 `MLPNet`, a callable
    that returns logits — its own forward followed by eb_policy_logp_from_logits.  Same numbers either way on an fp32 handle."""
    ar = _range(action_range)
    if isinstance(net, MLPNet):
        if net.output_dim < 2 or net.output_dim % 2:
            raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
        if _supported(net):
            x = net._in(_unwrap(obs).detach() if isinstance(_unwrap(obs), torch.Tensor) else obs)
            n = x.shape[0]
            out = _outputs(want, n, net.output_dim, net.device)
            _fused(net, x, _actions(actions, n, net.output_dim // 2, net.device), ar, out)
            return {k: DevArray(v) for k, v in out.items()}
        logits = MLPNet.call(net, obs)
    else:
        logits = net(obs)
    return log_prob_from_logits(logits, actions, action_range, want)


class _LogProb(torch.autograd.Function):
    """(logp, logits) of a TrainableMLPNet: forward the fused launch, backward eb_policy_logp_vjp + eb_mlp_backward(head = 0)"""

    @staticmethod
    def forward(ctx, net, ar, actions, x, *params):
        net._sync()
        out = _outputs(('logits', 'z'), x.shape[0], net.output_dim, net.device)
        _fused(net, x, actions, ar, out)
        ctx.net, ctx.version = net, net._flat._version
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, out['logits'], out['z'])
        return out['logp'], out['logits']

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logp, g_logits_in):
        net, (x, logits, z) = ctx.net, ctx.saved_tensors
        if net._flat._version != ctx.version:
            raise RuntimeError('the weights of %s were modified in place between this forward and its backward (version %d, expected %d): '
                               'the gradient would be that of another network' % (net.name, net._flat._version, ctx.version))
        n_in = 4
        if g_logp is None and g_logits_in is None:
            return (None,) * (n_in + len(net._params))
        net._sync()
        n = x.shape[0]
        if g_logp is None:
            g_logits = g_logits_in.to(dtype=torch.float32).contiguous()
        else:
            g_logits = torch.empty_like(logits)
            gl = g_logp.to(dtype=torch.float32).contiguous()
            _call(net.api, 'eb_policy_logp_vjp',
                  C.byref(_args(net._stream(), n, net.output_dim, logits=logits, z=z, g_logp=gl, g_logits=g_logits)))
            if g_logits_in is not None:
                g_logits = g_logits + g_logits_in.to(dtype=torch.float32)
        need = C.c_size_t(0)
        net.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=net.device)
        g_obs = torch.empty_like(x) if ctx.needs_input_grad[n_in - 1] else None
        g_flat = torch.empty_like(net._flat) if any(ctx.needs_input_grad[n_in:]) else None
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        net.api.mlp_backward(net._h, n, p(x), p(g_logits), 0, C.c_float(0.0), p(ws), need.value, None, p(g_obs), p(g_flat), net._stream())
        grads = [None] * len(net._params) if g_flat is None else [g_flat[a:b].view(shape) for a, b, shape in net._slices]
        return (None,) * (n_in - 1) + (g_obs,) + tuple(grads)


def log_prob(net, obs, actions, action_range):
    """(logp [B], logits [B, 2 * act_dim]) of the TrainableMLPNet `net` at obs for GIVEN actions [B, act_dim], as torch tensors on the
    autograd graph: one node.  The gradient reaches obs, when it requires grad, and every parameter of the network; none goes to the
    actions.  Any torch function of the returned logits (an entropy bonus, a KL to stored logits) differentiates through the same node.
    Forward is one launch; backward is eb_policy_logp_vjp and one eb_mlp_backward."""
    from .policy_grad import TrainableMLPNet
    if not isinstance(net, TrainableMLPNet):
        raise TypeError('log_prob differentiates a TrainableMLPNet, got %s (log_prob_actions serves inference)' % type(net).__name__)
    if net.output_dim < 2 or net.output_dim % 2:
        raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
    x = net._graph_in(obs)
    if not _supported(net):
        net.api.check(-1)                                    # the C reason: an fp16 handle has no gradient
    a = _actions(actions, x.shape[0], net.output_dim // 2, net.device)
    return _LogProb.apply(net, _range(action_range), a, x, *net._params)


# ---- the contract in NumPy ----------------------------------------------------------------------------------------------------------
_f = np.float32
U_MAX = _f(1.0 - 2.0 ** -24)            # 0x1.fffffep-1f


def policy_logp_reference(logits, actions, action_range, g_logp=None, dtype=np.float32):
    """The contract of include/envbuild_policy_logp.h in NumPy -> (logp [n], z [n, act_dim], g_logits [n, out_dim] or None).

    logits [n, 2 * act_dim]: the activated outputs of the network; actions [n, act_dim]: given; action_range None or <= 0: no squashing.
    g_logits is the reverse pass for the cotangent g_logp [n], None when it is not given.
    dtype float32: the kernels' operations one by one — the deterministic exp / log on the single-rounding fmaf, the division IEEE's,
    logp summed in ascending a from +0.0: their bits.  dtype float64: the same formulas and the same clamp with the library functions
    (np.arctanh, np.log1p) — the yardstick the float32 run and the kernels are measured against."""
    dtype = np.dtype(dtype).type
    y = np.asarray(logits).astype(dtype)
    a = np.asarray(actions).astype(dtype)
    act_dim = y.shape[1] // 2
    mean, ls = y[:, :act_dim], y[:, act_dim:]
    f32 = dtype == np.float32
    ar = -1.0 if action_range is None else float(action_range)
    if f32:
        ar = float(np.float32(ar))                             # the entry takes a float: log_ar is the logarithm of that number
    U = dtype(U_MAX)
    with np.errstate(all='ignore'):
        x = a
        if ar > 0:
            u = a / dtype(ar)
            u = np.where(u > U, U, np.where(u < -U, -U, u))    # selects: a NaN travels
            if f32:
                x = _f(0.5) * (_log_det(_f(1) + u) - _log_det(_f(1) - u))
            else:
                x = np.arctanh(u)
        if f32:
            inv = _exp_det(-ls)
            z = (x - mean) * inv
            n_a = ((_f(-0.5) * z) * z - ls) - _f(0.9189385332)
        else:
            inv = np.exp(-ls)
            z = (x - mean) * inv
            n_a = (-0.5 * z * z - ls) - 0.5 * math.log(2.0 * math.pi)
        if ar > 0:
            ax = np.abs(x)
            if f32:
                c_a = _f(2) * ((_f(0.6931471806) - ax) - _log_det(_f(1) + _exp_det(_f(-2) * ax)))
                n_a = n_a - (_f(math.log(ar)) + c_a)
            else:
                c_a = 2.0 * ((math.log(2.0) - ax) - np.log1p(np.exp(-2.0 * ax)))
                n_a = n_a - (math.log(ar) + c_a)
        logp = np.zeros(len(y), dtype)
        for k in range(act_dim):
            logp = logp + n_a[:, k]
        g_y = None
        if g_logp is not None:
            g_lp = np.asarray(g_logp).astype(dtype).reshape(-1, 1)
            g_y = np.concatenate([g_lp * (z * inv), g_lp * (z * z - dtype(1))], axis=1).astype(dtype)
    return logp.astype(dtype), z.astype(dtype), g_y
