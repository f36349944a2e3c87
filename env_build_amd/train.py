"""One PPO minibatch as a fixed chain of library launches (include/envbuild_train.h, env_build_amd/csrc/eb_train.hip): the value loss
with its gradient in ONE launch, Adam / AdamW with global-norm clipping in TWO — the step count and the bias-correction powers live on
the device — and `PPOUpdate`, which strings them together with eb_ppo_surrogate, eb_mlp_forward, eb_mlp_backward and
eb_mlp_set_params_device.  `PPOUpdate.step()` makes no torch arithmetic, no host read, no allocation and no autograd, so it can be issued
eagerly or captured once (`PPOUpdate.capture()`) and replayed: a replayed graph takes the NEXT optimiser step.

`value_loss(values, ret, v_old=None, clip_v=0.0, scale=None)` -> (loss, g_values): eb_value_loss.
`Adam(params_or_nets, lr, betas, eps, weight_decay, max_grad_norm)`: eb_adam_step over torch tensors with `.grad` (one segment per
tensor, at most 32) or over `TrainableMLPNet`s (one segment per net: its flat weights and a flat gradient buffer).
`PPOUpdate(policy, value, n_rows, action_range, clip, ...)`: every buffer of a minibatch allocated once; filling `mb.*` is the caller's.

`value_loss_reference` and `adam_reference` restate the header's contract in NumPy; in float32 every operation is the kernels' — their
bits —, in float64 they are the yardstick.

The entries live in env_build_amd/lib/libenvbuild_train.so, a library of its own that is bound here on first use (TRAIN_PROTOTYPES):
libenvbuild_hip.so and _capi's tables stay as they are, and nothing but this module loads the training library.  There is no CPU path.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _capi
from . import ppo as _ppo
from .dynamics_and_models import DevArray, _dev, _stream, _unwrap

__all__ = ['value_loss', 'Adam', 'PPOUpdate', 'value_loss_reference', 'adam_reference', 'EbValueLossArgs', 'EbAdamSegment', 'EbAdamState',
           'EbAdamArgs', 'EB_TRAIN_ABI_VERSION', 'EB_TRAIN_MAX_SEGMENTS', 'EB_TRAIN_ADAM_PARTIALS', 'TRAIN_PROTOTYPES', 'train_api']

_P, _I, _F, _D = C.c_void_p, C.c_int32, C.c_float, C.c_double
EB_TRAIN_ABI_VERSION = 1
EB_TRAIN_MAX_SEGMENTS = 32
EB_TRAIN_ADAM_PARTIALS = 256
CHUNK = 1024                                                   # elements of one chunk of a segment (csrc/eb_train_device.h)
HEADER = 'envbuild_train.h'


class EbValueLossArgs(C.Structure):
    """eb_value_loss_args of include/envbuild_train.h"""
    _fields_ = [('n', _I), ('stride', _I), ('values', _P), ('ret', _P), ('v_old', _P), ('clip_v', _F), ('scale', _F), ('loss', _P),
                ('g_values', _P), ('stream', _P)]


class EbAdamSegment(C.Structure):
    """eb_adam_segment"""
    _fields_ = [('params', _P), ('grads', _P), ('m', _P), ('v', _P), ('count', C.c_int64)]


class EbAdamState(C.Structure):
    """eb_adam_state: 32 bytes on the device"""
    _fields_ = [('step', C.c_int64), ('b1t', _D), ('b2t', _D), ('gnorm', _F), ('coef', _F)]


class EbAdamArgs(C.Structure):
    """eb_adam_args"""
    _fields_ = [('n_segments', _I), ('segments', EbAdamSegment * EB_TRAIN_MAX_SEGMENTS), ('lr', _D), ('beta1', _D), ('beta2', _D),
                ('eps', _D), ('weight_decay', _D), ('max_grad_norm', _D), ('state', _P), ('partials', _P), ('stream', _P)]


# include/envbuild_train.h: name -> (restype, argtypes) for every symbol the header declares
TRAIN_PROTOTYPES = {
    'eb_train_abi_version': (C.c_int, []),
    'eb_train_last_error': (C.c_char_p, []),
    'eb_value_loss': (C.c_int, [C.POINTER(EbValueLossArgs)]),
    'eb_adam_step': (C.c_int, [C.POINTER(EbAdamArgs)]),
}


class TrainApi(object):
    """libenvbuild_train.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in TRAIN_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in TRAIN_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_train_abi_version()
        if v != EB_TRAIN_ABI_VERSION:
            raise _capi.EbError('%s: train ABI version %d, expected %d (include/%s)' % (path, v, EB_TRAIN_ABI_VERSION, HEADER))
        self.value_loss, self.adam_step = self.lib.eb_value_loss, self.lib.eb_adam_step

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_train_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(train): %s' % msg)
            raise _capi.EbError('envbuild(train) error %d: %s' % (rc, msg))


_train_api = None


def train_api():
    """The training library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls back —
    when it is absent or was built from other sources and cannot be rebuilt."""
    global _train_api
    if _train_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.train_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.TRAIN_LIB, _build.CSRC))
            try:
                _build.build_train()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.TRAIN_LIB, e))
        _train_api = TrainApi(_build.TRAIN_LIB)
    return _train_api


def _scalar(x, name, lowest=None):
    x = float(x)
    if x != x or (lowest is not None and x < lowest):
        raise ValueError('%s must be a number%s, got %r' % (name, '' if lowest is None else ' >= %g' % lowest, x))
    return x


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---- the value loss ---------------------------------------------------------------------------------------------------------------------
def value_loss(values, ret, v_old=None, clip_v=0.0, scale=None):
    """eb_value_loss: the value network's output values [n] or [n, 1], the returns ret [n] and, for the clipped loss, the values v_old [n]
    of the collection -> (loss [n], unscaled; g_values, shaped like values: the gradient of scale * sum(loss)) as DevArrays.  One launch.
    scale None: 1 / n."""
    v = _unwrap(values)
    if not (isinstance(v, torch.Tensor) and v.is_cuda):
        raise TypeError('values must live on the GPU (a DevArray or a device tensor): there is no CPU path')
    v = v.detach().to(dtype=torch.float32).contiguous()
    if v.dim() == 2 and v.shape[1] == 1:
        flat = v[:, 0]
    elif v.dim() == 1:
        flat = v
    else:
        raise ValueError('values must be [n] or [n, 1], got %s' % (tuple(v.shape),))
    n = flat.shape[0]
    r = _dev(_detached(ret), v.device)
    vo = None if v_old is None else _dev(_detached(v_old), v.device)
    if tuple(r.shape) != (n,) or (vo is not None and tuple(vo.shape) != (n,)):
        raise ValueError('ret and v_old must be [%d], got %s and %s' % (n, tuple(r.shape), None if vo is None else tuple(vo.shape)))
    sc = 1.0 / max(n, 1) if scale is None else _scalar(scale, 'scale')
    loss, g = torch.empty((n,), dtype=torch.float32, device=v.device), torch.empty_like(v)
    api = train_api()
    with torch.cuda.device(v.device):
        a = EbValueLossArgs(n=n, stride=1, values=_ptr(v), ret=_ptr(r), v_old=_ptr(vo), clip_v=_scalar(clip_v, 'clip_v', 0.0), scale=sc,
                            loss=_ptr(loss), g_values=_ptr(g), stream=_stream(v.device))
        api.check(api.value_loss(C.byref(a)))
    return DevArray(loss), DevArray(g)


def _detached(x):
    x = _unwrap(x)
    return x.detach() if isinstance(x, torch.Tensor) else x


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
class AdamState(object):
    """eb_adam_state on the device: `buffer` (4 x int64, zero: a valid start) and views of its fields as device tensors — step (int64),
    b1t, b2t (float64), gnorm, coef (float32), one element each.  Reading one is the caller's host read; step() makes none."""

    def __init__(self, device):
        self.buffer = torch.zeros((4,), dtype=torch.int64, device=device)
        f64, f32 = self.buffer.view(torch.float64), self.buffer.view(torch.float32)
        self.step, self.b1t, self.b2t, self.gnorm, self.coef = self.buffer[0:1], f64[1:2], f64[2:3], f32[6:7], f32[7:8]

    def host(self):
        """the five fields as Python numbers (one device-to-host copy)"""
        raw = self.buffer.cpu().numpy()
        return dict(step=int(raw[0]), b1t=float(raw.view(np.float64)[1]), b2t=float(raw.view(np.float64)[2]),
                    gnorm=raw.view(np.float32)[6], coef=raw.view(np.float32)[7])


class Adam(object):
    """Adam (weight_decay = 0) / AdamW (decoupled weight_decay) with global-norm gradient clipping (max_grad_norm <= 0, None or inf: off)
    as eb_adam_step: two launches per step(), whatever the number of parameters.

    params_or_nets: torch device tensors (float32, contiguous; the gradient of each is its `.grad` when step() is called, a tensor
    without one is skipped) — one segment per tensor, more than 32 raise ValueError — or `TrainableMLPNet`s — one segment per net, on the
    net's flat weight tensor and a flat gradient buffer `grads[i]` (eb_mlp_backward's g_params can write it directly; step() gathers the
    `.grad`s autograd left on the net's parameters into it when there are any).
    `state` (an AdamState) holds the step count, the powers of the betas and the last step's gnorm / coef on the device.
    step() makes no host read.  After it the version of every net's flat tensor has moved, so `_sync()` uploads the new weights before
    the next launch on the net, and a backward of a graph built before the step raises, as after any in-place write."""

    def __init__(self, params_or_nets, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        from .policy_grad import TrainableMLPNet
        items = list(params_or_nets)
        if not items:
            raise ValueError('Adam needs at least one parameter tensor or TrainableMLPNet')
        if len(items) > EB_TRAIN_MAX_SEGMENTS:
            raise ValueError('Adam takes at most %d segments (EB_TRAIN_MAX_SEGMENTS), got %d: pass TrainableMLPNets, or flat tensors'
                             % (EB_TRAIN_MAX_SEGMENTS, len(items)))
        self.nets = [x for x in items if isinstance(x, TrainableMLPNet)]
        if self.nets and len(self.nets) != len(items):
            raise TypeError('Adam takes tensors or TrainableMLPNets, not a mixture')
        self.params = [net._flat for net in self.nets] if self.nets else items
        for p in self.params:
            if not (isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise TypeError('every parameter must be a contiguous float32 device tensor (there is no CPU path)')
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise ValueError('all parameters must live on one device')
        self.lr, self.eps, self.weight_decay = _scalar(lr, 'lr', 0.0), _scalar(eps, 'eps', 0.0), _scalar(weight_decay, 'weight_decay', 0.0)
        self.beta1, self.beta2 = _scalar(betas[0], 'beta1', 0.0), _scalar(betas[1], 'beta2', 0.0)
        if self.beta1 >= 1.0 or self.beta2 >= 1.0:
            raise ValueError('betas must lie in [0, 1), got %r' % (betas,))
        self.max_grad_norm = 0.0 if max_grad_norm is None else _scalar(max_grad_norm, 'max_grad_norm')
        self.grads = [torch.zeros_like(p) for p in self.params] if self.nets else None
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.state = AdamState(self.device)
        self.partials = torch.zeros((EB_TRAIN_ADAM_PARTIALS,), dtype=torch.float64, device=self.device)
        self.api = train_api()
        self._args = EbAdamArgs(n_segments=len(self.params), lr=self.lr, beta1=self.beta1, beta2=self.beta2, eps=self.eps,
                                weight_decay=self.weight_decay, max_grad_norm=self.max_grad_norm, state=_ptr(self.state.buffer),
                                partials=_ptr(self.partials))
        for k, p in enumerate(self.params):
            seg = self._args.segments[k]
            seg.params, seg.m, seg.v, seg.count = _ptr(p), _ptr(self.m[k]), _ptr(self.v[k]), p.numel()
            if self.grads is not None:
                seg.grads = _ptr(self.grads[k])

    def _gather(self):
        """the `.grad`s autograd left on the nets' parameters, copied into the flat gradient buffers (a parameter without one: zeros)"""
        for net, flat in zip(self.nets, self.grads):
            if any(p.grad is not None for p in net._params):
                for p, (a, b, _shape) in zip(net._params, net._slices):
                    if p.grad is None:
                        flat[a:b].zero_()
                    else:
                        flat[a:b].copy_(p.grad.reshape(-1))

    def issue(self):
        """eb_adam_step on the current stream with the struct as it stands, and nothing else"""
        self._args.stream = _stream(self.device)
        self.api.check(self.api.adam_step(C.byref(self._args)))

    def bump(self):
        """tell torch that the nets' flat weight tensors were written: `_sync()` and the version guards of the autograd nodes see it"""
        for net in self.nets:
            torch.autograd.graph.increment_version(net._flat)

    def step(self, gather=True):
        if self.nets:
            if gather:
                self._gather()
        else:
            for k, p in enumerate(self.params):
                seg, g = self._args.segments[k], p.grad
                if g is None:
                    seg.count = 0
                    continue
                if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape):
                    raise TypeError('the gradient of parameter %d must be a contiguous float32 device tensor shaped like it' % k)
                seg.grads, seg.count = _ptr(g), p.numel()
        with torch.cuda.device(self.device):
            self.issue()
        if self.nets:
            self.bump()
        else:
            for p in self.params:
                torch.autograd.graph.increment_version(p)

    def zero_grad(self):
        if self.nets:
            for net in self.nets:
                for p in net._params:
                    p.grad = None
        else:
            for p in self.params:
                p.grad = None


# ---- one PPO minibatch ---------------------------------------------------------------------------------------------------------------------
class _Buffers(object):
    def __init__(self, **tensors):
        self.__dict__.update(tensors)


class PPOUpdate(object):
    """One PPO minibatch of `n_rows` rows for a policy and a value `TrainableMLPNet` as a fixed chain of 13 kernels on the current stream:

        eb_ppo_surrogate(policy)        rows.logp, ratio, surr, ent; the cotangent of the logits with scale = 1 / n_rows
        eb_mlp_backward(policy)         head = 0, into the policy's flat gradient                         (3 kernels)
        eb_mlp_forward(value)
        eb_value_loss                   rows.vloss; the cotangent of the values with scale = vf_coef / n_rows
        eb_mlp_backward(value)          into the value net's flat gradient                                (3 kernels)
        eb_adam_step                    over both nets, one global gradient norm                          (2 kernels)
        eb_mlp_set_params_device x 2    both inference handles current again

    Everything is allocated here, once: the staging buffers `mb.obs` [n, obs_dim], `mb.actions` [n, act_dim], `mb.logp_old`, `mb.adv`,
    `mb.ret`, `mb.v_old` [n] and `mb.adv_norm` [2] ((mean, 1 / std), (0, 1) as made), both backward workspaces, both flat gradients
    (`adam.grads`), the Adam state (`adam.state`) and the per-row outputs `rows.logp`, `rows.ratio`, `rows.surr`, `rows.ent`,
    `rows.vloss` [n].  Filling `mb.*` (torch.index_select(..., out=mb.obs), copy_) is the caller's job and sits outside the chain.
    clip_v None: the unclipped value loss (mb.v_old is not read).  step() makes no torch operation, no host read, no allocation and no
    autograd; weights written by someone else since the last upload are uploaded first (a host-side version compare)."""

    def __init__(self, policy, value, n_rows, action_range, clip, ent_coef=0.0, vf_coef=0.5, clip_v=None, lr=3e-4, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        from .policy_grad import TrainableMLPNet
        from .policy_sample import _range
        for net in (policy, value):
            if not isinstance(net, TrainableMLPNet):
                raise TypeError('PPOUpdate trains TrainableMLPNets, got %s' % type(net).__name__)
        if policy.output_dim < 2 or policy.output_dim % 2:
            raise ValueError('the policy network must have 2 * act_dim outputs, got %d' % policy.output_dim)
        if value.input_dim != policy.input_dim or value.device != policy.device:
            raise ValueError('policy and value must take the same observations on the same device')
        if not _ppo._supported(policy):
            policy.api.check(-1)                                 # the C reason: an fp16 handle has no gradient
        n = int(n_rows)
        if n < 1:
            raise ValueError('n_rows must be at least 1')
        self.policy, self.value, self.n, self.device, self.api = policy, value, n, policy.device, policy.api
        dev, f32 = self.device, torch.float32
        new = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        self.mb = _Buffers(obs=new(n, policy.input_dim), actions=new(n, policy.output_dim // 2), logp_old=new(n), adv=new(n), ret=new(n),
                           v_old=new(n), adv_norm=torch.tensor([0.0, 1.0], dtype=f32, device=dev))
        self.rows = _Buffers(logp=new(n), ratio=new(n), surr=new(n), ent=new(n), vloss=new(n))
        self.g_logits, self.values, self.g_values = new(n, policy.output_dim), new(n, value.output_dim), new(n, value.output_dim)
        self.adam = self._make_adam([policy, value], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self._ws = []
        for net in (policy, value):
            net._sync()                                          # a handle that has never been uploaded has no layers yet
            need = C.c_size_t(0)
            self.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
            self._ws.append((torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value))
        ent_coef = float(np.float32(_scalar(ent_coef, 'ent_coef')))
        self.vf_coef = _scalar(vf_coef, 'vf_coef')
        self._surrogate = _ppo.bind(self.api)['eb_ppo_surrogate']
        self._ppo_args = _ppo._args(None, n, 0, _range(action_range), _scalar(clip, 'clip', 0.0), ent_coef, 1.0 / n, obs=self.mb.obs,
                                    actions=self.mb.actions, logp_old=self.mb.logp_old, adv=self.mb.adv, adv_norm=self.mb.adv_norm,
                                    logp=self.rows.logp, ratio=self.rows.ratio, surr=self.rows.surr, ent=self.rows.ent,
                                    g_logits=self.g_logits)
        self._vl_args = EbValueLossArgs(n=n, stride=value.output_dim, values=_ptr(self.values), ret=_ptr(self.mb.ret),
                                        v_old=None if clip_v is None else _ptr(self.mb.v_old),
                                        clip_v=0.0 if clip_v is None else _scalar(clip_v, 'clip_v', 0.0), scale=self.vf_coef / n,
                                        loss=_ptr(self.rows.vloss), g_values=_ptr(self.g_values))
        self._train = train_api()

    def _make_adam(self, nets, **kw):
        """the optimiser of the chain: step() calls its issue() and bump() (env_build_amd.ctl.PPOUpdate puts a controlled one here)"""
        return Adam(nets, **kw)

    def step(self):
        """the chain, on the current stream"""
        pol, val, api, n = self.policy, self.value, self.api, self.n
        pol._sync()
        val._sync()
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            obs = self.mb.obs.data_ptr()
            self._ppo_args.stream = s
            api.check(self._surrogate(pol._h, C.byref(self._ppo_args)))
            (ws, need), g = self._ws[0], self.adam.grads[0]
            api.mlp_backward(pol._h, n, obs, self.g_logits.data_ptr(), 0, 0.0, ws.data_ptr(), need, None, None, g.data_ptr(), s)
            api.mlp_forward(val._h, n, obs, self.values.data_ptr(), s)
            self._vl_args.stream = s
            self._train.check(self._train.value_loss(C.byref(self._vl_args)))
            (ws, need), g = self._ws[1], self.adam.grads[1]
            api.mlp_backward(val._h, n, obs, self.g_values.data_ptr(), 0, 0.0, ws.data_ptr(), need, None, None, g.data_ptr(), s)
            self.adam.issue()
            self.adam.bump()
            for net in (pol, val):
                api.mlp_set_params_device(net._h, net._flat.data_ptr(), s)
                net._uploaded = net._flat._version

    def capture(self, keep_graph=False):
        """a torch.cuda.CUDAGraph of one step(): a linear chain of 13 kernel nodes on one stream.  Nothing runs during the capture;
        every replay is one minibatch on whatever `mb.*` holds then, and takes the next optimiser step.  keep_graph: the hipGraph
        stays readable (raw_cuda_graph()) after the instantiation.
        Replay it with `self.replay(graph)`.  A bare `graph.replay()` writes the flat weight tensors without torch knowing: the version
        bump is host code that ran once, at capture, so the version guards of the autograd nodes do not see the write, and a backward
        of a graph built before the replay would differentiate other weights where the eager step() raises.  The handles themselves
        stay current either way (the uploads are inside the graph)."""
        import gc
        self.policy._sync()
        self.value._sync()
        graph = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
        was = gc.isenabled()
        gc.disable()               # a collection inside the captured region may finalise a handle (hipFree): not a call to capture
        try:
            with torch.cuda.graph(graph):
                self.step()
        finally:
            if was:
                gc.enable()
        if keep_graph:
            graph.instantiate()
        return graph

    def replay(self, graph):
        """graph.replay() for a graph of capture(), and what step() does on the host after its launches: the version of both flat weight
        tensors moves (an older autograd graph's backward is refused, as after step()) and `_uploaded` follows it.  No host read."""
        graph.replay()
        self.adam.bump()
        for net in (self.policy, self.value):
            net._uploaded = net._flat._version


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def value_loss_reference(values, ret, v_old=None, clip_v=0.0, scale=None, dtype=np.float32):
    """eb_value_loss's contract in NumPy -> (loss, g).  scale None: 1 / n.  dtype float32: the kernel's operations one by one — its bits;
    float64: the same lines in double."""
    dtype = np.dtype(dtype).type
    v, r = np.asarray(values).astype(dtype).reshape(-1), np.asarray(ret).astype(dtype).reshape(-1)
    sc = dtype(1.0 / max(len(v), 1) if scale is None else scale)
    half = dtype(0.5)
    with np.errstate(all='ignore'):
        e = v - r
        l1 = e * e
        if v_old is None:
            return (half * l1).astype(dtype), (sc * e).astype(dtype)
        vo, c = np.asarray(v_old).astype(dtype).reshape(-1), dtype(clip_v)
        dv = v - vo
        cl = np.where(dv < -c, -c, np.where(dv > c, c, dv)).astype(dtype)
        vc = vo + cl
        e2 = vc - r
        l2 = e2 * e2
        inside = (dv >= -c) & (dv <= c)
        second = l2 > l1
        loss = half * np.where(second, l2, l1)
        g = sc * np.where(second, np.where(inside, e2, dtype(0)), e)
    return loss.astype(dtype), g.astype(dtype)


def adam_reference(params, grads, m, v, state=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                   gnorm=None, dtype=np.float32):
    """One eb_adam_step in NumPy on lists of arrays (one per segment) -> (params, m, v, state), all new.  state: dict(step, b1t, b2t,
    gnorm, coef) or None (the zero state); the powers are maintained by repeated double multiplication, not beta ** t.
    gnorm: the kernel's global norm, when the caller has it (the order of its sum is the kernel's own); None: the square root of the
    float64 sum of squares, rounded to dtype.
    dtype float32: the kernel's operations one by one — its bits given its gnorm; float64: the same lines in double, uniforms unrounded."""
    dtype = np.dtype(dtype).type
    f32 = dtype == np.float32
    params, grads, m, v = ([np.asarray(a).astype(dtype) for a in x] for x in (params, grads, m, v))
    st = dict(step=0, b1t=0.0, b2t=0.0) if state is None else dict(state)
    lr, b1, b2, eps, wd = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    was0 = st['step'] == 0
    b1t, b2t = (1.0 if was0 else float(st['b1t'])) * b1, (1.0 if was0 else float(st['b2t'])) * b2
    with np.errstate(all='ignore'):
        if gnorm is None:
            total = sum(float(np.sum(np.square(g.astype(np.float64)))) for g in grads)
            gnorm = dtype(np.sqrt(np.float64(total)))
        gnorm = dtype(gnorm)
        mx = 0.0 if max_grad_norm is None else float(max_grad_norm)
        coef = dtype(1)
        if mx > 0.0 and not math.isinf(mx):
            q = dtype(mx) / (gnorm + dtype(1e-6))
            coef = dtype(1) if q > dtype(1) else dtype(q)
        ss, sb = dtype(lr / (1.0 - b1t)), dtype(np.sqrt(np.float64(1.0 - b2t)))
        fb1, fb2, o1, o2, ep, lwd = dtype(b1), dtype(b2), dtype(1.0 - b1), dtype(1.0 - b2), dtype(eps), dtype(lr * wd)
        out_p, out_m, out_v = [], [], []
        for p, g, mm, vv in zip(params, grads, m, v):
            g = g * coef
            if wd != 0.0:
                p = p - lwd * p
            mm = fb1 * mm + o1 * g
            vv = fb2 * vv + (o2 * g) * g
            den = np.sqrt(vv) / sb + ep
            p = p - ss * (mm / den)
            out_p.append(p.astype(dtype))
            out_m.append(mm.astype(dtype))
            out_v.append(vv.astype(dtype))
    assert not f32 or all(a.dtype == np.float32 for a in out_p + out_m + out_v)
    return out_p, out_m, out_v, dict(step=st['step'] + 1, b1t=b1t, b2t=b2t, gnorm=gnorm, coef=coef)
