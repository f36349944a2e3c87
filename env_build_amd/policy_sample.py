"""The stochastic head of the policy on the GPU (include/envbuild_policy_sample.h, env_build_amd/csrc/eb_policy_sample.hip): the branch of
the reference's Policy4Toyota its trainers use (utils/policy.py:71-96) — a sample of MultivariateNormalDiag(mean, exp(log_std)) under
Affine(action_range) o Tanh, returned with its log_prob.

`sample_actions(net, obs, action_range, ...)` is the inference surface: network and sampling epilogue in ONE launch where
eb_policy_sample_supported says yes (an fp32 `MLPNet`), otherwise `net(obs)` followed by eb_policy_sample_from_logits (an fp16 `MLPNet`,
any callable policy that returns [B, 2 * act_dim] logits).  The Gaussian noise is a function of (seed, counter, row id) and never
exists in memory unless asked for; with `eps` given it is taken as is (eps = 0 gives the deterministic action the shield sees).
`sample(net, obs, action_range, ...)` is the training surface: one torch.autograd.Function on a `TrainableMLPNet` that returns
(actions, logp) on the graph; its backward is the reparameterised one (eps held fixed): eb_policy_sample_vjp, then
eb_mlp_backward(head = 0), with gradients to obs and to every parameter.
`sample_from_logits` / `sample_vjp` wrap the two elementwise entries.

`policy_sample_reference` and `policy_noise_reference` restate the header's contract in NumPy; in float32 every fused multiply-add is
libm's fmaf (one rounding), so they are what the kernels compute bit for bit.

The entries are bound here, on `hip_api().lib`, on first use (POLICY_SAMPLE_PROTOTYPES): _capi's tables are envbuild.h's and the nine
families', and stay so.  There is no CPU path.
"""
import ctypes as C
import ctypes.util
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi
from .dynamics_and_models import DevArray, _dev, _stream, _unwrap
from . import policy as _policy
from .policy import MLPNet

__all__ = ['sample_actions', 'sample_from_logits', 'sample_vjp', 'sample', 'policy_sample_reference', 'policy_noise_reference',
           'EB_POLICY_SAMPLE_ABI_VERSION', 'POLICY_SAMPLE_PROTOTYPES']

_P, _I, _U64, _F = C.c_void_p, C.c_int32, C.c_uint64, C.c_float

# include/envbuild_policy_sample.h: name -> (restype, argtypes) for every symbol the header declares
EB_POLICY_SAMPLE_ABI_VERSION = 1
HEADER = 'envbuild_policy_sample.h'
POLICY_SAMPLE_PROTOTYPES = {
    'eb_policy_sample_abi_version': (C.c_int, []),
    'eb_policy_sample_supported': (C.c_int, [_P, C.POINTER(_I)]),
    # (m, n, obs, eps, row_ids, seed, counter, action_range, actions, logp, logits_out, eps_out, stream)
    'eb_policy_sample': (C.c_int, [_P, _I, _P, _P, _P, _U64, _U64, _F, _P, _P, _P, _P, _P]),
    # (n, out_dim, logits, eps, row_ids, seed, counter, action_range, actions, logp, eps_out, stream)
    'eb_policy_sample_from_logits': (C.c_int, [_I, _I, _P, _P, _P, _U64, _U64, _F, _P, _P, _P, _P]),
    # (n, out_dim, logits, eps, action_range, g_actions, g_logp, g_logits, stream)
    'eb_policy_sample_vjp': (C.c_int, [_I, _I, _P, _P, _F, _P, _P, _P, _P]),
}


def bind(api):
    """name -> raw ctypes function for every entry of POLICY_SAMPLE_PROTOTYPES on `api` (a _capi.CApi), bound on first use; EbError when
    the library does not export them or speaks another version."""
    fns = api.__dict__.setdefault('_policy_sample_fns', {})
    if not fns:
        missing = [n for n in POLICY_SAMPLE_PROTOTYPES if not hasattr(api.lib, n)]
        if missing:
            raise _capi.EbError('%s (backend %r) does not export %s: this library has no stochastic policy head (include/%s is implemented '
                                'by the HIP library only; rebuild an older one)' % (api.path, api.backend, ', '.join(missing), HEADER))
        for n, (res, args) in POLICY_SAMPLE_PROTOTYPES.items():
            fn = getattr(api.lib, n)
            fn.restype, fn.argtypes = res, args
            fns[n] = fn
        v = fns['eb_policy_sample_abi_version']()
        if v != EB_POLICY_SAMPLE_ABI_VERSION:
            fns.clear()
            raise _capi.EbError('%s: policy-sample ABI version %d, expected %d (include/%s)' % (api.path, v, EB_POLICY_SAMPLE_ABI_VERSION, HEADER))
    return fns


def _call(api, name, *args):
    api.check(bind(api)[name](*args))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _range(action_range):
    ar = -1.0 if action_range is None else float(action_range)
    if ar != ar:
        raise ValueError('action_range is NaN')
    return ar


def _row_ids(row_ids, n, device):
    if row_ids is None:
        return None
    r = _unwrap(row_ids)
    if not isinstance(r, torch.Tensor):
        r = torch.from_numpy(np.ascontiguousarray(np.asarray(r).astype(np.uint32).view(np.int32)))     # ids are unsigned 32-bit numbers
    r = r.to(device=device, dtype=torch.int32).contiguous()
    if tuple(r.shape) != (n,):
        raise ValueError('row_ids must be [%d], got %s' % (n, tuple(r.shape)))
    return r


def _eps(eps, n, act_dim, device):
    if eps is None:
        return None
    e = _dev(eps, device)
    if tuple(e.shape) != (n, act_dim):
        raise ValueError('eps must be [%d, %d], got %s' % (n, act_dim, tuple(e.shape)))
    return e


_WANT = ('logp', 'logits', 'eps')


def _outputs(want, n, out_dim, device):
    unknown = [w for w in want if w not in _WANT]
    if unknown:
        raise ValueError('want: unknown output %r (of %r)' % (unknown[0], _WANT))
    shapes = {'actions': (n, out_dim // 2), 'logp': (n,), 'logits': (n, out_dim), 'eps': (n, out_dim // 2)}
    return {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in ('actions',) + tuple(w for w in _WANT if w in want)}


def _from_logits(api, logits, ar, eps, seed, counter, row_ids, out):
    n, out_dim = logits.shape
    _call(api, 'eb_policy_sample_from_logits', n, out_dim, _ptr(logits), _ptr(eps), _ptr(row_ids), int(seed), int(counter), ar,
          _ptr(out['actions']), _ptr(out.get('logp')), _ptr(out.get('eps')), _stream(logits.device))


def sample_from_logits(logits, action_range, eps=None, seed=0, counter=0, row_ids=None, want=('logp',)):
    """eb_policy_sample_from_logits: the sampling epilogue alone on [B, 2 * act_dim] logits (what `MLPNet.call` returns) ->
    {'actions': [B, act_dim], 'logp': [B], 'eps': [B, act_dim]} as DevArrays ('actions' and what `want` names)."""
    t = _unwrap(logits)
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError('logits must live on the GPU (a DevArray or a device tensor): there is no CPU path')
    t = t.detach().to(dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] < 2 or t.shape[1] % 2 or t.shape[1] > 32:
        raise ValueError('logits must be [B, 2 * act_dim] with act_dim in 1..16, got %s' % (tuple(t.shape),))
    n, out_dim = t.shape
    out = _outputs([w for w in want if w != 'logits'], n, out_dim, t.device)
    with torch.cuda.device(t.device):
        _from_logits(_capi.hip_api(), t, _range(action_range), _eps(eps, n, out_dim // 2, t.device), seed, counter,
                     _row_ids(row_ids, n, t.device), out)
    if 'logits' in want:
        out['logits'] = t
    return {k: DevArray(v) for k, v in out.items()}


def sample_vjp(logits, eps, action_range, g_actions=None, g_logp=None):
    """eb_policy_sample_vjp: the cotangent of the logits [B, 2 * act_dim] from those of the actions [B, act_dim] and of logp [B] (None:
    zeros), eps [B, act_dim] held fixed -> DevArray."""
    t = _unwrap(logits)
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError('logits must live on the GPU (a DevArray or a device tensor): there is no CPU path')
    t = t.detach().to(dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] < 2 or t.shape[1] % 2 or t.shape[1] > 32:
        raise ValueError('logits must be [B, 2 * act_dim] with act_dim in 1..16, got %s' % (tuple(t.shape),))
    n, out_dim = t.shape
    e = _eps(eps, n, out_dim // 2, t.device)
    if e is None:
        raise ValueError('eps is required: the reverse pass holds the noise of the forward fixed')
    ga = None if g_actions is None else _dev(g_actions, t.device)
    gl = None if g_logp is None else _dev(g_logp, t.device)
    if ga is not None and tuple(ga.shape) != (n, out_dim // 2) or gl is not None and tuple(gl.shape) != (n,):
        raise ValueError('g_actions must be [%d, %d] and g_logp [%d]' % (n, out_dim // 2, n))
    g = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _call(_capi.hip_api(), 'eb_policy_sample_vjp', n, out_dim, _ptr(t), _ptr(e), _range(action_range), _ptr(ga), _ptr(gl), _ptr(g),
              _stream(t.device))
    return DevArray(g)


def _supported(net):
    ok = C.c_int32(0)
    _call(net.api, 'eb_policy_sample_supported', net._handle, C.byref(ok))
    return bool(ok.value)


def _fused(net, x, ar, eps, seed, counter, row_ids, out):
    _call(net.api, 'eb_policy_sample', net._handle, x.shape[0], _ptr(x), _ptr(eps), _ptr(row_ids), int(seed), int(counter), ar,
          _ptr(out['actions']), _ptr(out.get('logp')), _ptr(out.get('logits')), _ptr(out.get('eps')), _stream(net.device))


def sample_actions(net, obs, action_range, eps=None, seed=0, counter=0, row_ids=None, want=('logp',)):
    """Actions a ~ action_range * tanh(N(mean, exp(log_std))) of the policy `net` at obs [B, obs_dim], with what `want` names of 'logp'
    (log pi(a | obs), [B]), 'logits' ([B, 2 * act_dim]) and 'eps' (the noise used, [B, act_dim]) -> {'actions': ..., ...} as DevArrays.

    eps [B, act_dim] given: taken as is.  eps None: drawn from (seed, counter, row id); row_ids [B] (unsigned 32-bit numbers, None: the
    row index) name the rows, so an env's draw does not depend on where it sits in the batch.  action_range None: no squashing.
    An fp32 `MLPNet` (a `TrainableMLPNet` included) takes the fused entry, one launch; any other policy — an fp16 `MLPNet`, a callable
    that returns logits — its own forward followed by eb_policy_sample_from_logits.  Same numbers either way on an fp32 handle."""
    ar = _range(action_range)
    if isinstance(net, MLPNet):
        if net.output_dim < 2 or net.output_dim % 2:
            raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
        if _supported(net):
            x = net._in(_unwrap(obs).detach() if isinstance(_unwrap(obs), torch.Tensor) else obs)
            n = x.shape[0]
            out = _outputs(want, n, net.output_dim, net.device)
            _fused(net, x, ar, _eps(eps, n, net.output_dim // 2, net.device), seed, counter, _row_ids(row_ids, n, net.device), out)
            return {k: DevArray(v) for k, v in out.items()}
        logits = MLPNet.call(net, obs)
    else:
        logits = net(obs)
    return sample_from_logits(logits, action_range, eps, seed, counter, row_ids, want)


class _Sample(torch.autograd.Function):
    """(actions, logp) of a TrainableMLPNet: forward the fused launch, backward eb_policy_sample_vjp + eb_mlp_backward(head = 0)"""

    @staticmethod
    def forward(ctx, net, ar, eps, seed, counter, row_ids, x, *params):
        net._sync()
        n = x.shape[0]
        out = _outputs(('logp', 'logits') if eps is not None else ('logp', 'logits', 'eps'), n, net.output_dim, net.device)
        _fused(net, x, ar, eps, seed, counter, row_ids, out)
        ctx.net, ctx.ar, ctx.version = net, ar, net._flat._version
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, out['logits'], eps if eps is not None else out['eps'])
        return out['actions'], out['logp']

    @staticmethod
    @once_differentiable
    def backward(ctx, g_actions, g_logp):
        net, (x, logits, eps) = ctx.net, ctx.saved_tensors
        if net._flat._version != ctx.version:
            raise RuntimeError('the weights of %s were modified in place between this forward and its backward (version %d, expected %d): '
                               'the gradient would be that of another network' % (net.name, net._flat._version, ctx.version))
        n_in = 7
        if g_actions is None and g_logp is None:
            return (None,) * (n_in + len(net._params))
        net._sync()
        n = x.shape[0]
        ga = None if g_actions is None else g_actions.to(dtype=torch.float32).contiguous()
        gl = None if g_logp is None else g_logp.to(dtype=torch.float32).contiguous()
        g_logits = torch.empty_like(logits)
        _call(net.api, 'eb_policy_sample_vjp', n, net.output_dim, _ptr(logits), _ptr(eps), ctx.ar, _ptr(ga), _ptr(gl), _ptr(g_logits),
              net._stream())
        need = C.c_size_t(0)
        net.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=net.device)
        g_obs = torch.empty_like(x) if ctx.needs_input_grad[n_in - 1] else None
        g_flat = torch.empty_like(net._flat) if any(ctx.needs_input_grad[n_in:]) else None
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        net.api.mlp_backward(net._h, n, p(x), p(g_logits), 0, C.c_float(0.0), p(ws), need.value, None, p(g_obs), p(g_flat), net._stream())
        grads = [None] * len(net._params) if g_flat is None else [g_flat[a:b].view(shape) for a, b, shape in net._slices]
        return (None,) * (n_in - 1) + (g_obs,) + tuple(grads)


def sample(net, obs, action_range, eps=None, seed=0, counter=0, row_ids=None):
    """(actions [B, act_dim], logp [B]) of the TrainableMLPNet `net` at obs, as torch tensors on the autograd graph: one node.  The
    reparameterised gradient (the noise — given, or drawn from (seed, counter, row id) — is held fixed) reaches obs, when it requires
    grad, and every parameter of the network.  Forward is one launch; backward is eb_policy_sample_vjp and one eb_mlp_backward."""
    from .policy_grad import TrainableMLPNet
    if not isinstance(net, TrainableMLPNet):
        raise TypeError('sample differentiates a TrainableMLPNet, got %s (sample_actions serves inference)' % type(net).__name__)
    if net.output_dim < 2 or net.output_dim % 2:
        raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % net.output_dim)
    x = net._graph_in(obs)
    n = x.shape[0]
    if not _supported(net):
        net.api.check(-1)                                    # the C reason: an fp16 handle has no gradient
    e = _eps(eps.detach() if isinstance(eps, torch.Tensor) else eps, n, net.output_dim // 2, net.device)
    return _Sample.apply(net, _range(action_range), e, int(seed), int(counter), _row_ids(row_ids, n, net.device), x, *net._params)


# ---- the contract in NumPy ----------------------------------------------------------------------------------------------------------
_libm = C.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fmaf.restype, _libm.fmaf.argtypes = C.c_float, [C.c_float, C.c_float, C.c_float]
_fmaf_obj = np.frompyfunc(_libm.fmaf, 3, 1)
_f = np.float32


def _fmaf(a, b, c):
    """fmaf on float32 arrays, ONE rounding: libm's, element by element (policy._fma32 goes through float64 and rounds twice)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, _f), np.asarray(b, _f), np.asarray(c, _f))
    return np.asarray(_fmaf_obj(a, b, c), dtype=_f).reshape(a.shape)


def _exp_det(x):
    """csrc/eb_mlp_device.h:exp_det on the single-rounding fmaf"""
    return _policy._exp_det(x, _fmaf)


def _tanh_det(x):
    """csrc/eb_mlp_device.h:tanh_det on the single-rounding fmaf"""
    return _policy._tanh_det(x, _fmaf)


def _log_det(x0):
    """csrc/eb_policy_sample_device.h:log_det (finite positive normal x; a NaN travels)"""
    x0 = np.ascontiguousarray(x0, _f)
    with np.errstate(all='ignore'):
        bits = x0.view(np.uint32)
        e0 = ((bits >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32) - 126
        m = ((bits & np.uint32(0x807fffff)) | np.uint32(0x3f000000)).view(_f)
        low = m < _f(0.707106781186547524)
        fe = np.where(low, e0 - 1, e0).astype(_f)
        x = np.where(low, (m + m) - _f(1), m - _f(1)).astype(_f)
        z = x * x
        p = np.full_like(x, 7.0376836292e-2)
        for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1,
                  -2.4999993993e-1, 3.3333331174e-1):
            p = _fmaf(p, x, _f(c))
        y = (p * x) * z
        y = _fmaf(_f(-2.12194440e-4), fe, y)
        y = _fmaf(_f(-0.5), z, y)
        r = _fmaf(_f(0.693359375), fe, x + y)
    return np.where(np.isnan(x0), x0, r).astype(_f)


def _sincos_det(x):
    """csrc/eb_device.h:sincos_det"""
    x = np.asarray(x, _f)
    with np.errstate(all='ignore'):
        kf = np.rint(x * _f(0.636619747)).astype(_f)
        # the device's v_cvt_i32_f32 (the oracle's cvt_i32_f32): saturating at -2^31 and 2^31 - 1, NaN -> 0
        k = np.clip(np.nan_to_num(kf.astype(np.float64), nan=0.0), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
        r = _fmaf(-kf, _f(1.5703125), x)
        r = _fmaf(-kf, _f(4.83751296997070312e-4), r)
        r = _fmaf(-kf, _f(7.54978995489188216e-8), r)
        z = r * r
        ps = _fmaf(_f(-1.9515295891e-4), z, _f(8.3321608736e-3))
        ps = _fmaf(ps, z, _f(-1.6666654611e-1))
        s = _fmaf(r * z, ps, r)
        pc = _fmaf(_f(2.443315711809948e-5), z, _f(-1.388731625493765e-3))
        pc = _fmaf(pc, z, _f(4.166664568298827e-2))
        c = _fmaf(z * z, pc, _fmaf(_f(-0.5), z, _f(1)))
        odd, neg = (k & 1) != 0, (k & 2) != 0
        a = np.where(odd, c, s)
        b = np.where(odd, -s, c)
    return np.where(neg, -a, a).astype(_f), np.where(neg, -b, b).astype(_f)


_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _splitmix64(z):
    """csrc/eb_env_device.h:splitmix64 on uint64 arrays (arithmetic modulo 2^64)"""
    z = np.asarray(z, np.uint64) + _GOLDEN
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u01(key, idx):
    """csrc/eb_env_device.h:u01: the top 24 bits of splitmix64(key + GOLDEN * idx) -> [0, 1)"""
    return (_splitmix64(key + _GOLDEN * np.asarray(idx, np.uint64)) >> np.uint64(40)).astype(_f) * _f(5.9604644775390625e-8)


def policy_noise_reference(row_ids, act_dim, seed, counter):
    """The noise of include/envbuild_policy_sample.h: eps [n, act_dim] float32 for the rows named row_ids (unsigned 32-bit numbers) under
    (seed, counter) — what eb_policy_sample draws when eps is NULL, bit for bit."""
    ids = np.asarray(row_ids).astype(np.uint32).astype(np.uint64).reshape(-1, 1)
    act_dim = int(act_dim)
    P = (act_dim + 1) // 2
    with np.errstate(over='ignore'):
        key = _splitmix64(np.array([int(seed) % 2 ** 64], np.uint64) + _GOLDEN * np.array([int(counter) % 2 ** 64], np.uint64))
        idx = np.uint64(2) * (np.arange(P, dtype=np.uint64).reshape(1, -1) + np.uint64(P) * ids)
        u = _f(1) - _u01(key, idx)
        v = _u01(key, idx + np.uint64(1))
    with np.errstate(all='ignore'):
        r = np.sqrt(_f(-2) * _log_det(u)).astype(_f)
        sn, cs = _sincos_det(_f(6.2831855) * v)
        eps = np.empty((len(ids), 2 * P), _f)
        eps[:, 0::2] = r * cs
        eps[:, 1::2] = r * sn
    return np.ascontiguousarray(eps[:, :act_dim])


def policy_sample_reference(logits, eps, action_range, g_actions=None, g_logp=None, dtype=np.float32):
    """The contract of include/envbuild_policy_sample.h in NumPy -> (actions [n, act_dim], logp [n], g_logits [n, out_dim] or None).

    logits [n, 2 * act_dim]: the activated outputs of the network; eps [n, act_dim]; action_range None or <= 0: no squashing.
    g_logits is the reverse pass for the cotangents g_actions [n, act_dim] / g_logp [n] (None: zeros), None when neither is given.
    dtype float32: the kernels' operations one by one — the deterministic exp / tanh / log, every fused multiply-add one rounding
    (libm's fmaf), logp summed in ascending a from +0.0: their bits.  dtype float64: the same formulas with the library functions —
    the yardstick the float32 run and the kernels are measured against."""
    dtype = np.dtype(dtype).type
    y = np.asarray(logits, np.float32).astype(dtype)
    e = np.asarray(eps, np.float32).astype(dtype)
    act_dim = y.shape[1] // 2
    mean, ls = y[:, :act_dim], y[:, act_dim:]
    f32 = dtype == np.float32
    ar = -1.0 if action_range is None else float(action_range)
    if f32:
        ar = float(np.float32(ar))                             # the entry takes a float: log_ar is the logarithm of that number
    with np.errstate(all='ignore'):
        if f32:
            std = _exp_det(ls)
            x = _fmaf(std, e, mean)
            n_a = ((_f(-0.5) * e) * e - ls) - _f(0.9189385332)
        else:
            std = np.exp(ls)
            x = mean + std * e
            n_a = (-0.5 * e * e - ls) - 0.5 * math.log(2.0 * math.pi)
        t = None
        if ar > 0:
            ax = np.abs(x)
            if f32:
                t = _tanh_det(x)
                c_a = _f(2) * ((_f(0.6931471806) - ax) - _log_det(_f(1) + _exp_det(_f(-2) * ax)))
                n_a = n_a - (_f(math.log(ar)) + c_a)
            else:
                t = np.tanh(x)
                c_a = 2.0 * ((math.log(2.0) - ax) - np.log1p(np.exp(-2.0 * ax)))
                n_a = n_a - (math.log(ar) + c_a)
            actions = dtype(ar) * t
        else:
            actions = x.copy()
        logp = np.zeros(len(y), dtype)
        for a in range(act_dim):
            logp = logp + n_a[:, a]
        g_y = None
        if g_actions is not None or g_logp is not None:
            g_a = np.zeros_like(e) if g_actions is None else np.asarray(g_actions, np.float32).astype(dtype)
            g_lp = (np.zeros(len(y), dtype) if g_logp is None else np.asarray(g_logp, np.float32).astype(dtype)).reshape(-1, 1)
            if ar > 0:
                da = dtype(ar) * (dtype(1) - t * t)
                s = g_a * da + g_lp * (dtype(2) * t)
            else:
                s = g_a
            g_y = np.concatenate([s + np.zeros_like(e), s * (std * e) - g_lp], axis=1).astype(dtype)
    return actions.astype(dtype), logp.astype(dtype), g_y
