"""The two controls of a PPO update phase, on the DEVICE, so that a captured graph obeys them at every replay (include/envbuild_ctl.h,
env_build_amd/csrc/eb_ctl.hip): the learning-rate factor of the iteration, read from a table the caller fills (eb_ctl_begin, ONE launch),
and the approximate-KL stop (eb_kl_stop, TWO launches; eb_adam_step_ctl, TWO launches, which takes the step at lr * factor or — once
stopped — nothing at all).

`UpdateControl(device, lr_table=None, target_kl=None, kl_factor=1.5, max_slots=1024)`: the 32-byte control block, the table, the scratch
and the per-slot log on the device.
`Adam(train.Adam)`: issue() is [eb_kl_stop when target_kl is set] + eb_adam_step_ctl.
`PPOUpdate(train.PPOUpdate)`: the minibatch chain with the controlled Adam — 13 kernels, 15 with target_kl.
`PPOEpochs(epoch.PPOEpochs)`: eb_ctl_begin, then the parent's chain — 4 + 15 * epochs * minibatches kernels with normalisation,
4 + 17 * epochs * minibatches with target_kl; one linear graph, captured and replayed as the parent's.

A captured graph cannot branch: after a stop the remaining minibatches of the iteration still run their forward, backward and log, and
re-upload the unchanged weights.  The gain is the trust region, not time.

`begin_reference`, `kl_stop_reference` and `adam_ctl_reference` restate the header's contract in NumPy and carry the kernels' bits.

The entries live in env_build_amd/lib/libenvbuild_ctl.so, a library of its own that is bound here on first use (CTL_PROTOTYPES): the
other four libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from . import epoch as _epoch
from . import train as _train
from .dynamics_and_models import _stream

__all__ = ['UpdateControl', 'Adam', 'PPOUpdate', 'PPOEpochs', 'begin_reference', 'kl_stop_reference', 'adam_ctl_reference', 'EbUpdateCtl',
           'EbCtlBeginArgs', 'EbKlStopArgs', 'EbAdamCtlArgs', 'EB_CTL_ABI_VERSION', 'EB_CTL_KL_BLOCKS', 'CTL_PROTOTYPES', 'ctl_api']

_P, _I, _L, _F, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
EB_CTL_ABI_VERSION = 1
EB_CTL_KL_BLOCKS = 64
HEADER = 'envbuild_ctl.h'
FIELDS = ('iteration', 'lr_scale', 'stopped', 'slot', 'stopped_at', 'last_kl')


class EbUpdateCtl(C.Structure):
    """eb_update_ctl of include/envbuild_ctl.h: 32 bytes on the device"""
    _fields_ = [('iteration', C.c_uint64), ('lr_scale', _F), ('stopped', C.c_uint32), ('slot', _I), ('stopped_at', _I), ('last_kl', _D)]


class EbCtlBeginArgs(C.Structure):
    """eb_ctl_begin_args"""
    _fields_ = [('ctl', _P), ('lr_table', _P), ('n_table', _I), ('stream', _P)]


class EbKlStopArgs(C.Structure):
    """eb_kl_stop_args"""
    _fields_ = [('n', _L), ('logp', _P), ('logp_old', _P), ('limit', _D), ('ctl', _P), ('partials', _P), ('log', _P), ('max_slots', _I),
                ('stream', _P)]


class EbAdamCtlArgs(C.Structure):
    """eb_adam_ctl_args: eb_adam_args by value, then the control block"""
    _fields_ = [('adam', _train.EbAdamArgs), ('ctl', _P)]


# include/envbuild_ctl.h: name -> (restype, argtypes) for every symbol the header declares
CTL_PROTOTYPES = {
    'eb_ctl_abi_version': (C.c_int, []),
    'eb_ctl_last_error': (C.c_char_p, []),
    'eb_ctl_begin': (C.c_int, [C.POINTER(EbCtlBeginArgs)]),
    'eb_kl_stop': (C.c_int, [C.POINTER(EbKlStopArgs)]),
    'eb_adam_step_ctl': (C.c_int, [C.POINTER(EbAdamCtlArgs)]),
}


class CtlApi(object):
    """libenvbuild_ctl.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in CTL_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in CTL_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_ctl_abi_version()
        if v != EB_CTL_ABI_VERSION:
            raise _capi.EbError('%s: ctl ABI version %d, expected %d (include/%s)' % (path, v, EB_CTL_ABI_VERSION, HEADER))
        self.ctl_begin, self.kl_stop, self.adam_step_ctl = self.lib.eb_ctl_begin, self.lib.eb_kl_stop, self.lib.eb_adam_step_ctl

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_ctl_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(ctl): %s' % msg)
            raise _capi.EbError('envbuild(ctl) error %d: %s' % (rc, msg))


_ctl_api = None


def ctl_api():
    """The control library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls back —
    when it is absent or was built from other sources and cannot be rebuilt."""
    global _ctl_api
    if _ctl_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.ctl_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.CTL_LIB, _build.CSRC))
            try:
                _build.build_ctl()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.CTL_LIB, e))
        _ctl_api = CtlApi(_build.CTL_LIB)
    return _ctl_api


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fields_of(raw):
    """the 32 bytes of an eb_update_ctl (a uint8 array) -> dict of the six fields"""
    c = EbUpdateCtl.from_buffer_copy(np.ascontiguousarray(raw, np.uint8).tobytes())
    return dict(iteration=int(c.iteration), lr_scale=np.float32(c.lr_scale), stopped=int(c.stopped), slot=int(c.slot),
                stopped_at=int(c.stopped_at), last_kl=float(c.last_kl))


# ---- the control block -------------------------------------------------------------------------------------------------------------------
class UpdateControl(object):
    """eb_update_ctl on the device and what goes with it, allocated once: `buffer` (4 x int64, zero: valid before the first begin()),
    `table` (lr_table as a float32 device tensor, or None: the factor is 1), `partials` (64 doubles of scratch) and `log_buffer`
    [max_slots, 2] float64 = (kl, applied) per minibatch of the iteration.  target_kl None: no KL stop; otherwise an iteration's optimiser
    steps end at the first minibatch whose approximate KL is not <= `limit` = kl_factor * target_kl (Spinning Up's 1.5).
    begin() issues eb_ctl_begin on the current stream; host() and log() are the caller's host reads, nothing else here makes one."""

    def __init__(self, device, lr_table=None, target_kl=None, kl_factor=1.5, max_slots=1024):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise TypeError('UpdateControl lives on the GPU: there is no CPU path')
        self.max_slots = int(max_slots)
        if self.max_slots < 0:
            raise ValueError('max_slots must be >= 0')
        self.table = None
        if lr_table is not None:
            t = np.asarray(lr_table.detach().cpu().numpy() if isinstance(lr_table, torch.Tensor) else lr_table, np.float32).reshape(-1)
            if t.size < 1 or np.isnan(t).any():
                raise ValueError('lr_table must hold at least one factor and no NaN')
            self.table = torch.from_numpy(t.copy()).to(self.device)
        self.limit = None
        if target_kl is not None:
            self.limit = _train._scalar(kl_factor, 'kl_factor') * _train._scalar(target_kl, 'target_kl')
        self.buffer = torch.zeros((4,), dtype=torch.int64, device=self.device)
        self.device = self.buffer.device                         # with its index: 'cuda' is the current device
        self.partials = torch.zeros((EB_CTL_KL_BLOCKS,), dtype=torch.float64, device=self.device)
        self.log_buffer = torch.zeros((max(self.max_slots, 1), 2), dtype=torch.float64, device=self.device)
        if self.table is not None:
            self.table = self.table.to(self.device)
        self.api = ctl_api()
        self._begin = EbCtlBeginArgs(ctl=_ptr(self.buffer), lr_table=_ptr(self.table), n_table=0 if self.table is None else self.table.numel())

    def begin(self):
        """eb_ctl_begin on the current stream: the iteration's factor, the stop cleared"""
        with torch.cuda.device(self.device):
            self._begin.stream = _stream(self.device)
            self.api.check(self.api.ctl_begin(C.byref(self._begin)))

    def kl_args(self, logp, logp_old, n):
        """eb_kl_stop_args of this control on two [n] float32 device tensors (the stream is set at the call)"""
        if self.limit is None:
            raise ValueError('this UpdateControl has no target_kl')
        for t in (logp, logp_old):
            _epoch._f32(t, 'logp and logp_old', (n,))
        return EbKlStopArgs(n=n, logp=_ptr(logp), logp_old=_ptr(logp_old), limit=self.limit, ctl=_ptr(self.buffer),
                            partials=_ptr(self.partials), log=_ptr(self.log_buffer), max_slots=self.max_slots)

    def host(self):
        """the six fields (one device-to-host copy)"""
        return _fields_of(self.buffer.cpu().numpy().view(np.uint8))

    def log(self):
        """(kl, applied) per slot of the current iteration -> dict of two arrays [min(slot, max_slots)] (two device-to-host copies)"""
        n = min(self.host()['slot'], self.max_slots)
        raw = self.log_buffer.cpu().numpy()[:n]
        return dict(kl=raw[:, 0].copy(), applied=raw[:, 1].astype(np.int64))


# ---- the controlled optimiser ------------------------------------------------------------------------------------------------------------
class Adam(_train.Adam):
    """train.Adam under an UpdateControl: issue() is eb_adam_step_ctl — the step at lr * control's factor, or nothing once stopped —
    preceded by eb_kl_stop on the tensors `watch(logp, logp_old)` named when the control has a target_kl.  Everything else (segments,
    state, step(), bump()) is the parent's; the struct the parent fills is the `adam` member of eb_adam_ctl_args, in place."""

    def __init__(self, params_or_nets, control, **kw):
        if not isinstance(control, UpdateControl):
            raise TypeError('ctl.Adam needs an UpdateControl, got %s' % type(control).__name__)
        super().__init__(params_or_nets, **kw)
        if control.device != self.device:
            raise ValueError('the control block must live on the device of the parameters')
        self.control, self.capi = control, control.api
        self._cargs = EbAdamCtlArgs(adam=self._args, ctl=_ptr(control.buffer))
        self._args = self._cargs.adam                             # a view: what the parent writes into it is what the entry reads
        self._kl = None

    def watch(self, logp, logp_old):
        """the minibatch's log-probabilities under the current and the collecting policy, [n] float32 device tensors read at every issue()"""
        self._kl = self.control.kl_args(logp, logp_old, int(logp.numel()))

    def issue(self):
        """[eb_kl_stop] + eb_adam_step_ctl on the current stream with the structs as they stand, and nothing else"""
        s = _stream(self.device)
        if self.control.limit is not None:
            if self._kl is None:
                raise ValueError('the control has a target_kl: name the log-probabilities with watch(logp, logp_old) first')
            self._kl.stream = s
            self.capi.check(self.capi.kl_stop(C.byref(self._kl)))
        self._args.stream = s
        self.capi.check(self.capi.adam_step_ctl(C.byref(self._cargs)))


class PPOUpdate(_train.PPOUpdate):
    """train.PPOUpdate with the controlled Adam: the same chain, eb_adam_step replaced by [eb_kl_stop on rows.logp and mb.logp_old] +
    eb_adam_step_ctl — 13 kernels, 15 with target_kl.  The KL is taken after the surrogate and before the optimiser, on the weights
    before this minibatch's step.  control None: one is made from lr_table, target_kl, kl_factor and max_slots.  Opening the iteration
    (control.begin()) is the caller's, or ctl.PPOEpochs'."""

    def __init__(self, policy, value, n_rows, action_range, clip, control=None, lr_table=None, target_kl=None, kl_factor=1.5, max_slots=1024,
                 **kw):
        if control is None:
            control = UpdateControl(policy.device, lr_table=lr_table, target_kl=target_kl, kl_factor=kl_factor, max_slots=max_slots)
        elif lr_table is not None or target_kl is not None:
            raise ValueError('pass a control, or lr_table / target_kl to make one, not both')
        self.control = control
        super().__init__(policy, value, n_rows, action_range, clip, **kw)

    def _make_adam(self, nets, **kw):
        adam = Adam(nets, self.control, **kw)
        if self.control.limit is not None:
            adam.watch(self.rows.logp, self.mb.logp_old)
        return adam


class PPOEpochs(_epoch.PPOEpochs):
    """epoch.PPOEpochs over a ctl.PPOUpdate: step() is eb_ctl_begin followed by the parent's chain — 4 + 15 * epochs * minibatches
    kernels with normalize, 4 + 17 * epochs * minibatches with target_kl — one linear graph; capture() and replay() are the parent's.
    Every replay opens the next iteration: the next factor of the table, the stop cleared.  log() adds `applied` [epochs, minibatches]
    (1: that minibatch's optimiser step was taken), `stopped_at` (the slot e * minibatches + k that stopped the iteration, or -1) and
    `lr_scale`."""

    def __init__(self, update, data, epochs, minibatches, **kw):
        if not isinstance(update, PPOUpdate):
            raise TypeError('ctl.PPOEpochs drives a ctl.PPOUpdate, got %s' % type(update).__name__)
        super().__init__(update, data, epochs, minibatches, **kw)
        self.control = update.control
        if self.control.limit is not None and self.control.max_slots < self.epochs * self.minibatches:
            raise ValueError('the control logs %d slots, %d epochs of %d minibatches need %d'
                             % (self.control.max_slots, self.epochs, self.minibatches, self.epochs * self.minibatches))

    def step(self):
        """eb_ctl_begin and the whole chain, on the current stream"""
        self.control.begin()
        super().step()

    def log(self):
        out = super().log()
        st, slots = self.control.host(), self.epochs * self.minibatches
        applied = np.ones(slots, np.int64)
        if self.control.limit is not None:
            applied = self.control.log_buffer.cpu().numpy()[:slots, 1].astype(np.int64)
        out.update(applied=applied.reshape(self.epochs, self.minibatches), stopped_at=st['stopped_at'], lr_scale=st['lr_scale'])
        return out


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def _zero_ctl():
    return dict(iteration=0, lr_scale=np.float32(0.0), stopped=0, slot=0, stopped_at=0, last_kl=0.0)


def begin_reference(ctl=None, lr_table=None):
    """eb_ctl_begin in NumPy: ctl a dict of the six fields or None (the zero-filled block) -> a new dict"""
    c = _zero_ctl() if ctl is None else dict(ctl)
    it = int(c['iteration'])
    scale = np.float32(1.0)
    if lr_table is not None:
        table = np.asarray(lr_table, np.float32).reshape(-1)
        if table.size < 1:
            raise ValueError('lr_table must hold at least one factor')
        scale = table[min(it, table.size - 1)]
    return dict(iteration=it + 1, lr_scale=np.float32(scale), stopped=0, slot=0, stopped_at=-1, last_kl=0.0)


def kl_stop_reference(ctl, logp, logp_old, limit, log=None):
    """eb_kl_stop in NumPy -> (the control block after it, a new dict; kl).  The sum is eb_ppo_log's field 4 in `epoch.ppo_log_reference`'s
    order and the blocks are added in ascending order, as `epoch.fold_log` does: kl is fold_log's approx_kl of the same rows, bit for
    bit.  log: a float64 array [max_slots, 2] written in place, or None.  n = 0 leaves ctl alone and returns (ctl, None)."""
    limit = float(limit)
    if limit != limit:
        raise ValueError('limit is NaN')
    c = dict(ctl)
    lp, lo = np.asarray(logp, np.float32).reshape(-1), np.asarray(logp_old, np.float32).reshape(-1)
    if lp.size != lo.size:
        raise ValueError('logp and logp_old must have one length')
    n = lp.size
    if n == 0:
        return c, None
    blocks = _epoch.ppo_log_reference(logp=lp, logp_old=lo)[:, 4]
    total = blocks[0]
    with np.errstate(all='ignore'):
        for b in range(1, EB_CTL_KL_BLOCKS):
            total = total + blocks[b]
        kl = np.float64(total) / np.float64(n)
    stop_now = not (kl <= limit)
    s = int(c['slot'])
    if not c['stopped'] and stop_now:
        c['stopped'], c['stopped_at'] = 1, s
    if log is not None and 0 <= s < log.shape[0]:
        log[s, 0], log[s, 1] = kl, 0.0 if c['stopped'] else 1.0
    c['slot'], c['last_kl'] = s + 1, float(kl)
    return c, float(kl)


def adam_ctl_reference(ctl, params, grads, m, v, state=None, lr=1e-3, **kw):
    """eb_adam_step_ctl in NumPy on `train.adam_reference` -> (params, m, v, state), all new.  Stopped: the inputs, as they are.  Not
    stopped: adam_reference at lr * (double)lr_scale."""
    if ctl['stopped']:
        dtype = np.dtype(kw.get('dtype', np.float32)).type
        st = dict(step=0, b1t=0.0, b2t=0.0) if state is None else dict(state)
        return ([np.asarray(a).astype(dtype) for a in params], [np.asarray(a).astype(dtype) for a in m],
                [np.asarray(a).astype(dtype) for a in v], st)
    return _train.adam_reference(params, grads, m, v, state, lr=float(lr) * float(np.float32(ctl['lr_scale'])), **kw)
