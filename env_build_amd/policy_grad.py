"""A trainable `MLPNet`: the policy network's backward on the GPU (include/envbuild_mlp_grad.h, env_build_amd/csrc/eb_policy_grad.hip)
behind torch autograd, with the weights living in ONE flat device tensor that any torch optimiser steps.

`TrainableMLPNet` takes `MLPNet`'s constructor arguments.  `call(x)` / `mode(x, action_range)` return torch tensors on the autograd
graph: forward is eb_mlp_forward / eb_policy_run_batch, backward one eb_mlp_backward — the gradient of exactly the function the
inference handle evaluates.  The handle is brought up to date with eb_mlp_set_params_device whenever the flat tensor has been written
since the last upload (its `_version`): no host copy, no synchronisation, one policy.  The same handle serves the shield,
`policy_rollout` and `HierarchicalDecision`, at either precision; differentiating needs precision 'fp32'.

`rollout_loss` is the ADP loss of a whole closed-loop rollout under a `TrainableMLPNet` as ONE autograd node: value and parameter
gradient come from eb_policy_rollout_grad (include/envbuild_policy_rollout_grad.h) in its forward.  `rollout_loss_sampled` is the
maximum-entropy form under the stochastic head, J = sum of cost + w_logp * sum of log pi, through eb_policy_rollout_sample
(include/envbuild_policy_rollout_sample.h).

`mlp_backward_reference` restates the header's contract in NumPy.  There is no CPU path for the network itself.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi
from .dynamics_and_models import _dev
from .policy import MLPNet, _act_det, _tanh_det

__all__ = ['TrainableMLPNet', 'mlp_backward_reference', 'rollout_loss', 'rollout_loss_sampled']


def _act(act, x, dtype):
    if dtype == np.float32:
        return _act_det(act, x)
    with np.errstate(all='ignore'):
        if act == 'relu':
            return np.where(x > 0, x, 0.0)
        if act == 'elu':
            return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
        if act == 'tanh':
            return np.tanh(x)
    return x


def _derivative(act, y):
    """the derivative of an activation from its OUTPUT y, one operation each"""
    one = y.dtype.type(1)
    if act == 'relu':
        return np.where(y > 0, one, y.dtype.type(0))
    if act == 'elu':
        return np.where(y > 0, one, y + one)
    if act == 'tanh':
        return one - y * y
    return np.ones_like(y)


def _product(a, b, dtype, start=None):
    """start + a @ b: in float64 as one matrix product; in float32 with float32 products added one by one in ascending order of the
    reduction index (with `start`, the forward's chain: every step one fused multiply-add, through float64)."""
    if dtype == np.float64:
        out = a @ b
        return out if start is None else out + start
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32) if start is None else np.broadcast_to(start, (a.shape[0], b.shape[1])).astype(np.float32)
    with np.errstate(all='ignore'):
        for k in range(a.shape[1]):
            if start is None:
                acc = acc + a[:, k:k + 1] * b[k:k + 1, :]
            else:
                acc = (a[:, k:k + 1].astype(np.float64) * b[k:k + 1, :].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def mlp_backward_reference(layers, obs, g, hidden_act, out_act, obs_scale=None, head=0, action_range=1.0, dtype=np.float32):
    """The contract of include/envbuild_mlp_grad.h in NumPy: -> (out, g_obs, g_params), what eb_mlp_backward writes up to the order of
    each backward sum.

    layers: [(kernel [in, out], bias [out]), ...]; obs [n, in]; g: the cotangent of `out` — [n, out_dim] with head 0 (logits),
    [n, out_dim // 2] with head 1 (actions = action_range * tanh(mean), or the mean itself with action_range <= 0 or None).
    g_params is the list Model.get_weights() would have: [d kernel0, d bias0, d kernel1, ...].

    dtype float32: the forward is the kernel's chain (bias, then one fused multiply-add per input in ascending k; the deterministic
    float32 activations), every backward product is float32 and every backward sum float32 in ascending order of its index.
    dtype float64: the same formulas in float64 with the library activations — the yardstick the float32 run and the kernel are measured
    against."""
    dtype = np.dtype(dtype).type
    layers = [(np.asarray(w, np.float32).astype(dtype), np.asarray(b, np.float32).astype(dtype)) for w, b in layers]
    x = np.asarray(obs, np.float32).astype(dtype)
    g = np.asarray(g, np.float32).astype(dtype)
    scale = None if obs_scale is None else np.asarray(obs_scale, np.float32).astype(dtype)
    ar = -1.0 if action_range is None else float(action_range)
    with np.errstate(all='ignore'):
        if scale is not None:
            x = x * scale
        xs = [x]
        for L, (w, b) in enumerate(layers):
            pre = _product(xs[-1], w, dtype, start=b)
            xs.append(_act(out_act if L == len(layers) - 1 else hidden_act, pre, dtype))
        y = xs.pop()
        if head == 0:
            out, d = y, g * _derivative(out_act, y)
        else:
            act_dim = y.shape[1] // 2
            mean = y[:, :act_dim]
            d = np.zeros_like(y)
            if ar > 0:
                t = _tanh_det(mean) if dtype == np.float32 else np.tanh(mean)
                out = dtype(ar) * t
                d[:, :act_dim] = (g * dtype(ar)) * (dtype(1) - t * t) * _derivative(out_act, mean)
            else:
                out = mean.copy()
                d[:, :act_dim] = g * _derivative(out_act, mean)
        g_params = [None] * (2 * len(layers))
        for L in range(len(layers) - 1, -1, -1):
            g_params[2 * L] = _product(xs[L].T, d, dtype)
            g_params[2 * L + 1] = _product(np.ones((1, len(d)), dtype), d, dtype)[0]
            d = _product(d, layers[L][0].T, dtype)
            d = d * _derivative(hidden_act, xs[L]) if L > 0 else (d if scale is None else d * scale)
    return out.astype(dtype), d.astype(dtype), [a.astype(dtype) for a in g_params]


class _Evaluate(torch.autograd.Function):
    """call / mode of a TrainableMLPNet: forward through the inference entry, backward through eb_mlp_backward"""

    @staticmethod
    def forward(ctx, net, head, action_range, x, *params):
        net._sync()
        n = x.shape[0]
        out = torch.empty((n, net.output_dim if head == 0 else net.output_dim // 2), dtype=torch.float32, device=net.device)
        if head == 0:
            net.api.mlp_forward(net._h, n, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), net._stream())
        else:
            net.api.policy_run_batch(net._h, n, C.c_void_p(x.data_ptr()), C.c_float(action_range), C.c_void_p(out.data_ptr()), net._stream())
        ctx.net, ctx.head, ctx.action_range, ctx.version = net, head, action_range, net._flat._version
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        net, (x,) = ctx.net, ctx.saved_tensors
        if net._flat._version != ctx.version:
            raise RuntimeError('the weights of %s were modified in place between this forward and its backward (version %d, expected %d): '
                               'the gradient would be that of another network' % (net.name, net._flat._version, ctx.version))
        net._sync()
        n = x.shape[0]
        g = g.to(dtype=torch.float32).contiguous()
        need = C.c_size_t(0)
        net.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))       # refuses an fp16 handle with the C reason
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=net.device)
        g_obs = torch.empty_like(x) if ctx.needs_input_grad[3] else None
        g_flat = torch.empty_like(net._flat) if any(ctx.needs_input_grad[4:]) else None
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        net.api.mlp_backward(net._h, n, p(x), p(g), ctx.head, C.c_float(ctx.action_range), p(ws), need.value, None, p(g_obs), p(g_flat),
                             net._stream())
        grads = [None] * len(net._params) if g_flat is None else [g_flat[a:b].view(shape) for a, b, shape in net._slices]
        return (None, None, None, g_obs) + tuple(grads)


class TrainableMLPNet(MLPNet):
    """`MLPNet` with a backward.  The parameters are views of one flat device tensor in Keras order (kernel0 [in, out], bias0, ...), each a
    leaf that requires grad: `parameters()` goes to any torch optimiser.  `call` / `mode` return torch tensors on the autograd graph."""

    def __init__(self, input_dim, num_hidden_layers, num_hidden_units, hidden_activation, output_dim, **kwargs):
        self._h = None
        self._flat = None
        MLPNet.__init__(self, input_dim, num_hidden_layers, num_hidden_units, hidden_activation, output_dim, **kwargs)

    # the inference handle, current: whoever launches on it (the shield, policy_rollout, HierarchicalDecision) sees the latest weights
    @property
    def _handle(self):
        if self._h is not None:
            self._sync()
        return self._h

    @_handle.setter
    def _handle(self, value):
        self._h = value

    def __del__(self):
        try:
            if self._h is not None:
                self.api.lib.eb_mlp_destroy(self._h)
        except Exception:
            pass

    def _shapes(self):
        dims = [self.input_dim] + [self.num_hidden_units] * self.num_hidden_layers + [self.output_dim]
        return [s for L in range(self.num_hidden_layers + 1) for s in ((dims[L], dims[L + 1]), (dims[L + 1],))]

    def _create(self):
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        cfg = _capi.EbMlpConfig(_capi.EB_ABI_VERSION, self.input_dim, self.num_hidden_layers, self.num_hidden_units, self.output_dim,
                                _capi.ACT_ID[self.hidden_activation], _capi.ACT_ID[self.output_activation], index)
        m = C.c_void_p()
        self.api.check(self.api.lib.eb_mlp_create(C.byref(cfg), C.byref(m)))
        self._h = m
        if self.precision != 'fp32':
            self.api.mlp_set_precision(m, _capi.MLP_PRECISION_ID[self.precision])
        count = C.c_int64(0)
        self.api.mlp_param_count(m, C.byref(count))
        self._flat = torch.zeros((count.value,), dtype=torch.float32, device=self.device)
        self._slices, at = [], 0
        for shape in self._shapes():
            size = int(np.prod(shape))
            self._slices.append((at, at + size, shape))
            at += size
        assert at == count.value
        with torch.no_grad():
            self._params = [self._flat[a:b].view(shape) for a, b, shape in self._slices]
        for t in self._params:
            t.requires_grad_(True)
        self._uploaded = None

    def parameters(self):
        return list(self._params)

    def _sync(self):
        """eb_mlp_set_params_device when the flat tensor has been written since the last upload; stream-ordered, nothing waits"""
        if self._uploaded != self._flat._version:
            self.api.mlp_set_params_device(self._h, C.c_void_p(self._flat.data_ptr()), self._stream())
            self._uploaded = self._flat._version

    # -- weights ------------------------------------------------------------------------------
    def get_weights(self):
        flat = self._flat.detach().cpu().numpy()
        return [flat[a:b].reshape(shape).copy() for a, b, shape in self._slices]

    def set_weights(self, weights):
        weights = [np.ascontiguousarray(a, np.float32) for a in weights]
        shapes = self._shapes()
        if len(weights) != len(shapes):
            raise ValueError('expected %d arrays (kernel, bias per Dense layer)' % len(shapes))
        for a, shape in zip(weights, shapes):
            if a.shape != tuple(shape):
                raise ValueError('expected shapes %s, got %s' % (shapes, [w.shape for w in weights]))
        if self._flat is None:
            self._create()
        with torch.no_grad():
            self._flat.copy_(torch.from_numpy(np.concatenate([a.ravel() for a in weights])))

    def set_obs_scale(self, obs_scale):
        self._obs_scale = None if obs_scale is None else np.ascontiguousarray(obs_scale, np.float32)
        if self._obs_scale is not None and self._obs_scale.shape != (self.input_dim,):
            raise ValueError('obs_scale must have %d entries' % self.input_dim)
        self.api.mlp_set_obs_scale(self._h, None if self._obs_scale is None else self._obs_scale.ctypes.data)

    def _rebuild(self):        # MLPNet's host path: this class never rebuilds its handle
        raise NotImplementedError

    # -- forward ------------------------------------------------------------------------------
    def _graph_in(self, x):
        t = x if isinstance(x, torch.Tensor) else _dev(x, self.device)
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.dim() != 2 or t.shape[1] != self.input_dim:
            raise ValueError('input must be [B, %d], got %s' % (self.input_dim, tuple(t.shape)))
        return t

    def call(self, x, **kwargs):
        return _Evaluate.apply(self, 0, 0.0, self._graph_in(x), *self._params)

    __call__ = call

    def mode(self, x, action_range):
        return _Evaluate.apply(self, 1, -1.0 if action_range is None else float(action_range), self._graph_in(x), *self._params)


class _RolloutLoss(torch.autograd.Function):
    """J = sum over envs of the rollout's weighted cost; the entry runs in forward and leaves dJ/dtheta for backward"""

    @staticmethod
    def forward(ctx, model, net, steps, w5, action_range, fused, *params):
        from .policy_rollout import _composed_grad, _fused_grad
        net._sync()
        run = _fused_grad if fused else _composed_grad
        out = run(model, net, -1.0 if action_range is None else float(action_range), steps, w5, ('cost', 'g_params'))
        ctx.g_flat = out['g_params']
        ctx.slices = net._slices
        return out['cost'].sum()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        flat = ctx.g_flat * g
        return (None,) * 6 + tuple(flat[a:b].view(shape) for a, b, shape in ctx.slices)


def rollout_loss(model, net, obs0, ref_idx, horizon, w5, action_range=1.0, fused=None):
    """J = sum over envs and steps of out5 weighted by w5, for the closed-loop rollout of `horizon` steps of `model` (a 'training'-mode
    EnvironmentModel / DifferentiableEnvironmentModel) under the TrainableMLPNet `net` from obs0 [B, D] with paths ref_idx [B]: a scalar
    tensor on the autograd graph whose backward hands upstream * dJ/dtheta to the network's parameters.  ADP's loss
    (examples/adp_policy_gradient.py:rollout_loss with lam) is w5 = (-1, lam, 0, 0, 0) / (horizon * B).

    One autograd node: eb_policy_rollout_grad runs in the forward (three launches whatever the horizon) and the gradient is complete
    when forward returns.  A handle whose flat tensor was written since its last upload is refreshed first, as every launch on a
    TrainableMLPNet is.  Weights modified between this forward and its backward do not matter here — unlike call / mode, whose
    backward recomputes — because nothing is recomputed: the gradient is that of the weights the forward ran with.
    fused=None takes the one-call entry where eb_policy_rollout_grad_supported says yes, the composed loop of single entries
    elsewhere (policy_rollout.policy_rollout_grad's rule)."""
    from . import policy_rollout as pr
    if not isinstance(net, TrainableMLPNet):
        raise TypeError('rollout_loss differentiates a TrainableMLPNet, got %s' % type(net).__name__)
    steps = int(horizon)
    if steps < 1:
        raise ValueError('horizon must be at least 1')
    w5 = pr._w5(w5)
    model.reset(obs0.detach() if isinstance(obs0, torch.Tensor) else obs0, ref_idx)
    if fused is None:
        ok = C.c_int32(0)
        model.api.policy_rollout_grad_supported(model.handle, net._handle, C.byref(ok))
        fused = bool(ok.value)
    return _RolloutLoss.apply(model, net, steps, w5, action_range, bool(fused), *net._params)


class _RolloutLossSampled(torch.autograd.Function):
    """J = sum of cost + w_logp * sum of logp of the stochastic rollout; the entry runs in forward and leaves dJ/dtheta for backward"""

    @staticmethod
    def forward(ctx, model, net, steps, w5, w_logp, action_range, eps, seed, counter, fused, *params):
        from .policy_rollout import _composed_sample, _fused_sample
        net._sync()
        run = _fused_sample if fused else _composed_sample
        out = run(model, net, -1.0 if action_range is None else float(action_range), steps, w5, w_logp, eps, seed, counter, None,
                  ('cost', 'logp', 'g_params'))
        ctx.g_flat = out['g_params']
        ctx.slices = net._slices
        ctx.mark_non_differentiable(out['logp_steps'])
        return out['cost'].sum() + w_logp * out['logp_steps'].sum(), out['logp_steps']

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_logp):
        flat = ctx.g_flat * g
        return (None,) * 10 + tuple(flat[a:b].view(shape) for a, b, shape in ctx.slices)


def rollout_loss_sampled(model, net, obs0, ref_idx, horizon, w5, w_logp, seed, counter, eps=None, action_range=1.0, fused=None,
                         return_logp=False):
    """J = sum over envs of cost + w_logp * sum over envs and steps of log pi(a_t | obs_t), for the closed-loop rollout of `horizon`
    steps of `model` under the STOCHASTIC head of the TrainableMLPNet `net`: step t samples with (seed, counter + t), or takes eps
    [horizon, B, 2] as its noise.  A scalar tensor on the autograd graph whose backward hands upstream * dJ/dtheta — the
    reparameterised gradient, the noise held fixed — to the network's parameters.  Maximum-entropy ADP is w5 = (-1, lam, 0, 0, 0) /
    (horizon * B) and w_logp = alpha / (horizon * B).  return_logp: also logp_steps [horizon, B] (not differentiable).

    One autograd node: eb_policy_rollout_sample runs in the forward (three launches whatever the horizon) and the gradient is complete
    when forward returns; the `_sync()` / `_version` rule is rollout_loss's.  fused=None takes the one-call entry where
    eb_policy_rollout_sample_supported says yes, the composed loop of single entries elsewhere."""
    from . import policy_rollout as pr
    if not isinstance(net, TrainableMLPNet):
        raise TypeError('rollout_loss_sampled differentiates a TrainableMLPNet, got %s' % type(net).__name__)
    steps = int(horizon)
    if steps < 1:
        raise ValueError('horizon must be at least 1')
    w5 = pr._w5(w5)
    model.reset(obs0.detach() if isinstance(obs0, torch.Tensor) else obs0, ref_idx)
    B = pr._unwrap(model.obses).shape[0]
    e = None
    if eps is not None:
        e = (eps if isinstance(eps, torch.Tensor) else torch.as_tensor(eps)).detach().to(device=model.device, dtype=torch.float32).contiguous()
        if tuple(e.shape) != (steps, B, 2):
            raise ValueError('eps must be [%d, %d, 2], got %s' % (steps, B, tuple(e.shape)))
    if fused is None:
        ok = C.c_int32(0)
        pr._sample_call(model.api, 'eb_policy_rollout_sample_supported', model.handle, net._handle, C.byref(ok))
        fused = bool(ok.value)
    loss, logp = _RolloutLossSampled.apply(model, net, steps, w5, float(w_logp), action_range, e, int(seed), int(counter), bool(fused),
                                           *net._params)
    return (loss, logp) if return_logp else loss
