"""The update phase of a PPO iteration as ONE linear chain of library launches (include/envbuild_epoch.h, env_build_amd/csrc/eb_epoch.hip):
the minibatch gather under a keyed shuffle whose permutation never exists in memory (ONE launch for all six tensors of a minibatch),
the two floats of the advantage normalisation (TWO launches), the per-minibatch logging sums (ONE launch) and the shuffle's iteration
counter on the device — and `PPOEpochs`, which strings them around `train.PPOUpdate.step()` for epochs x minibatches minibatches.
`PPOEpochs.step()` makes no torch operation, no host read, no allocation and no autograd, so it can be issued eagerly or captured once
(`PPOEpochs.capture()`) and replayed once per iteration: a replayed graph takes the next optimiser steps under the next permutations.

`gather(sources, dests, offset, count, perm=None, seed=0, epoch=0, counter=None, index_out=None)`: eb_minibatch_gather.
`adv_stats(x, eps=1e-8, out=None)` -> [mean, 1 / (std + eps)] on the device: eb_adv_stats.
`ppo_log(rows, logp_old, clip, out)`: eb_ppo_log into out [64, 8] doubles; `fold_log(out)` folds a host copy into the usual figures.
`index_reference`, `adv_stats_reference` and `ppo_log_reference` restate the header's contract in NumPy, in the kernels' own order.

The entries live in env_build_amd/lib/libenvbuild_epoch.so, a library of its own that is bound here on first use (EPOCH_PROTOTYPES):
the other two libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from .dynamics_and_models import _stream

__all__ = ['gather', 'adv_stats', 'ppo_log', 'fold_log', 'PPOEpochs', 'index_reference', 'adv_stats_reference', 'ppo_log_reference',
           'EbGatherSource', 'EbGatherArgs', 'EbAdvStatsArgs', 'EbPpoLogArgs', 'EbEpochAdvanceArgs', 'EB_EPOCH_ABI_VERSION',
           'EB_EPOCH_MAX_SOURCES', 'EB_EPOCH_MAX_WIDTH', 'EB_EPOCH_GATHER_ROWS', 'EB_EPOCH_PARTIALS', 'EB_EPOCH_LOG_BLOCKS',
           'EB_EPOCH_LOG_FIELDS', 'EPOCH_PROTOTYPES', 'epoch_api']

_P, _I, _L, _U, _F, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
EB_EPOCH_ABI_VERSION = 1
EB_EPOCH_MAX_SOURCES = 8
EB_EPOCH_MAX_WIDTH = 4096
EB_EPOCH_GATHER_ROWS = 32
EB_EPOCH_PARTIALS = 256
EB_EPOCH_LOG_BLOCKS = 64
EB_EPOCH_LOG_FIELDS = 8
THREADS = 256                                                  # of every kernel (csrc/eb_epoch_device.h)
CHUNK = 1024                                                   # elements of one chunk of the statistics
GOLDEN = 0x9E3779B97F4A7C15
HEADER = 'envbuild_epoch.h'
_M64 = (1 << 64) - 1


class EbGatherSource(C.Structure):
    """eb_gather_source of include/envbuild_epoch.h"""
    _fields_ = [('src', _P), ('dst', _P), ('width', _I)]


class EbGatherArgs(C.Structure):
    """eb_gather_args"""
    _fields_ = [('n_total', _L), ('offset', _L), ('count', _L), ('n_sources', _I), ('sources', EbGatherSource * EB_EPOCH_MAX_SOURCES),
                ('perm', _P), ('perm_bytes', _I), ('seed', _U), ('epoch', _U), ('counter', _P), ('index_out', _P), ('stream', _P)]


class EbAdvStatsArgs(C.Structure):
    """eb_adv_stats_args"""
    _fields_ = [('n', _L), ('x', _P), ('eps', _D), ('out', _P), ('std_out', _P), ('partials', _P), ('stream', _P)]


class EbPpoLogArgs(C.Structure):
    """eb_ppo_log_args"""
    _fields_ = [('n', _L), ('logp', _P), ('logp_old', _P), ('ratio', _P), ('surr', _P), ('ent', _P), ('vloss', _P), ('clip', _F),
                ('out', _P), ('stream', _P)]


class EbEpochAdvanceArgs(C.Structure):
    """eb_epoch_advance_args"""
    _fields_ = [('counter', _P), ('by', _U), ('stream', _P)]


# include/envbuild_epoch.h: name -> (restype, argtypes) for every symbol the header declares
EPOCH_PROTOTYPES = {
    'eb_epoch_abi_version': (C.c_int, []),
    'eb_epoch_last_error': (C.c_char_p, []),
    'eb_minibatch_gather': (C.c_int, [C.POINTER(EbGatherArgs)]),
    'eb_adv_stats': (C.c_int, [C.POINTER(EbAdvStatsArgs)]),
    'eb_ppo_log': (C.c_int, [C.POINTER(EbPpoLogArgs)]),
    'eb_epoch_advance': (C.c_int, [C.POINTER(EbEpochAdvanceArgs)]),
}


class EpochApi(object):
    """libenvbuild_epoch.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in EPOCH_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in EPOCH_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_epoch_abi_version()
        if v != EB_EPOCH_ABI_VERSION:
            raise _capi.EbError('%s: epoch ABI version %d, expected %d (include/%s)' % (path, v, EB_EPOCH_ABI_VERSION, HEADER))
        self.minibatch_gather, self.adv_stats = self.lib.eb_minibatch_gather, self.lib.eb_adv_stats
        self.ppo_log, self.epoch_advance = self.lib.eb_ppo_log, self.lib.eb_epoch_advance

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_epoch_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(epoch): %s' % msg)
            raise _capi.EbError('envbuild(epoch) error %d: %s' % (rc, msg))


_epoch_api = None


def epoch_api():
    """The epoch library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls back —
    when it is absent or was built from other sources and cannot be rebuilt."""
    global _epoch_api
    if _epoch_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.epoch_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.EPOCH_LIB, _build.CSRC))
            try:
                _build.build_epoch()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.EPOCH_LIB, e))
        _epoch_api = EpochApi(_build.EPOCH_LIB)
    return _epoch_api


def _ptr(t):
    return None if t is None else t.data_ptr()


def _f32(t, what, shape=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise TypeError('%s must be a contiguous float32 device tensor (there is no CPU path)' % what)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s, got %s' % (what, tuple(shape), tuple(t.shape)))
    return t


def _width(t, what):
    if t.dim() not in (1, 2):
        raise ValueError('%s must be [rows] or [rows, width], got %s' % (what, tuple(t.shape)))
    return 1 if t.dim() == 1 else int(t.shape[1])


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def _gather_args(sources, dests, offset, count, perm, seed, epoch, counter, index_out):
    sources, dests = list(sources), list(dests)
    if len(sources) != len(dests) or not 1 <= len(sources) <= EB_EPOCH_MAX_SOURCES:
        raise ValueError('gather takes 1 .. %d sources and as many destinations, got %d and %d' % (EB_EPOCH_MAX_SOURCES, len(sources), len(dests)))
    n_total, count = int(sources[0].shape[0]), int(count)
    a = EbGatherArgs(n_total=n_total, offset=int(offset), count=count, n_sources=len(sources), seed=int(seed) & _M64, epoch=int(epoch) & _M64)
    for k, (s, d) in enumerate(zip(sources, dests)):
        w = _width(_f32(s, 'source %d' % k), 'source %d' % k)
        if s.shape[0] != n_total or s.device != sources[0].device:
            raise ValueError('every source must have %d rows on one device' % n_total)
        _f32(d, 'destination %d' % k)
        if d.device != s.device or d.numel() < count * w or (d.dim() == 2 and d.shape[1] != w) or d.dim() not in (1, 2):
            raise ValueError('destination %d must hold %d rows of %d floats, got %s' % (k, count, w, tuple(d.shape)))
        a.sources[k].src, a.sources[k].dst, a.sources[k].width = _ptr(s), _ptr(d), w
    if perm is not None:
        if not (isinstance(perm, torch.Tensor) and perm.is_cuda and perm.dtype in (torch.int32, torch.int64) and perm.is_contiguous()
                and perm.dim() == 1 and perm.shape[0] >= int(offset) + count):
            raise TypeError('perm must be a contiguous int32 or int64 device tensor of at least offset + count elements')
        a.perm, a.perm_bytes = _ptr(perm), perm.element_size()
    if counter is not None:
        if not (isinstance(counter, torch.Tensor) and counter.is_cuda and counter.dtype == torch.int64 and counter.numel() >= 1):
            raise TypeError('counter must be an int64 device tensor')
        a.counter = _ptr(counter)
    if index_out is not None:
        if not (isinstance(index_out, torch.Tensor) and index_out.is_cuda and index_out.dtype == torch.int32 and index_out.is_contiguous()
                and index_out.numel() >= count):
            raise TypeError('index_out must be a contiguous int32 device tensor of at least count elements')
        a.index_out = _ptr(index_out)
    return a


def gather(sources, dests, offset, count, perm=None, seed=0, epoch=0, counter=None, index_out=None):
    """eb_minibatch_gather: destination row r < count of every pair (sources[k] [n_total] or [n_total, width], dests[k]) takes source row
    perm[offset + r] — perm an int32 or int64 device tensor — or, without perm, index(key(seed, epoch, *counter), n_total, offset + r):
    the keyed shuffle, `index_reference(n_total, seed, epoch, base)[offset + r]`.  counter: an int64 device tensor read by the kernel.
    index_out: an int32 device tensor that receives the source rows.  ONE launch on the current stream, up to 8 pairs."""
    a = _gather_args(sources, dests, offset, count, perm, seed, epoch, counter, index_out)
    api, dev = epoch_api(), sources[0].device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.minibatch_gather(C.byref(a)))


def adv_stats(x, eps=1e-8, out=None, std_out=None):
    """eb_adv_stats: x [n] (n >= 2) -> out [2] = (mean, 1 / (std + eps)), the unbiased standard deviation as torch.std — what
    eb_ppo_args.adv_norm reads; std_out [1], when given, receives the standard deviation.  out is allocated when not given, the 512
    doubles of scratch always (PPOEpochs holds its own).  TWO launches."""
    x = _f32(x, 'x')
    dev = x.device
    out = torch.empty((2,), dtype=torch.float32, device=dev) if out is None else _f32(out, 'out', (2,))
    if std_out is not None:
        _f32(std_out, 'std_out', (1,))
    partials = torch.empty((2 * EB_EPOCH_PARTIALS,), dtype=torch.float64, device=dev)
    api = epoch_api()
    with torch.cuda.device(dev):
        a = EbAdvStatsArgs(n=x.numel(), x=_ptr(x), eps=float(eps), out=_ptr(out), std_out=_ptr(std_out), partials=_ptr(partials),
                           stream=_stream(dev))
        api.check(api.adv_stats(C.byref(a)))
    return out


def _log_args(rows, logp_old, clip, out, n=None):
    get = (lambda k: rows.get(k)) if isinstance(rows, dict) else (lambda k: getattr(rows, k, None))
    given = {k: get(k) for k in ('logp', 'ratio', 'surr', 'ent', 'vloss')}
    given['logp_old'] = logp_old
    sizes = {int(t.numel()) for t in given.values() if t is not None}
    if n is None:
        if len(sizes) != 1:
            raise ValueError('ppo_log needs at least one input, all of one length; got lengths %s' % sorted(sizes))
        n = sizes.pop()
    for k, t in given.items():
        if t is not None:
            _f32(t, k, (n,))
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and out.is_contiguous()
            and out.numel() == EB_EPOCH_LOG_BLOCKS * EB_EPOCH_LOG_FIELDS):
        raise TypeError('out must be a contiguous float64 device tensor of %d x %d' % (EB_EPOCH_LOG_BLOCKS, EB_EPOCH_LOG_FIELDS))
    return EbPpoLogArgs(n=n, clip=float(clip), out=_ptr(out), **{k: _ptr(t) for k, t in given.items()})


def ppo_log(rows, logp_old, clip, out):
    """eb_ppo_log: the per-row outputs of a minibatch (rows.logp, .ratio, .surr, .ent, .vloss — `PPOUpdate.rows`, or a dict; a missing one
    contributes 0) and logp_old -> out [64, 8] float64 on the device, the per-block sums `fold_log` reads.  ONE launch, no host read."""
    a = _log_args(rows, logp_old, clip, out)
    api, dev = epoch_api(), out.device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.ppo_log(C.byref(a)))
    return out


def fold_log(out):
    """out [..., 64, 8] (a HOST copy of eb_ppo_log's blocks) -> dict of arrays [...]: policy_loss (= -mean surr), value_loss, entropy,
    clip_fraction, approx_kl, max_ratio_dev, nonfinite_rows, rows.  The blocks are added in ascending order."""
    out = np.asarray(out, np.float64)
    if out.shape[-2:] != (EB_EPOCH_LOG_BLOCKS, EB_EPOCH_LOG_FIELDS):
        raise ValueError('fold_log takes [..., %d, %d], got %s' % (EB_EPOCH_LOG_BLOCKS, EB_EPOCH_LOG_FIELDS, out.shape))
    total = out[..., 0, :].copy()
    for b in range(1, EB_EPOCH_LOG_BLOCKS):
        total = total + out[..., b, :]
    top = out[..., :, 5].max(axis=-1)
    n = total[..., 7]
    with np.errstate(all='ignore'):
        return dict(policy_loss=-(total[..., 0] / n), value_loss=total[..., 1] / n, entropy=total[..., 2] / n, clip_fraction=total[..., 3] / n,
                    approx_kl=total[..., 4] / n, max_ratio_dev=top, nonfinite_rows=total[..., 6], rows=n)


# ---- epochs x minibatches ------------------------------------------------------------------------------------------------------------------
_FIELDS = ('obs', 'actions', 'logp_old', 'adv', 'ret', 'v_old')


class PPOEpochs(object):
    """The update phase of one PPO iteration — `epochs` passes over `minibatches` minibatches of `update.n` rows — on the current stream:

        eb_adv_stats(data.adv -> update.mb.adv_norm)                       when normalize                    (2 kernels)
        for every epoch e and minibatch k:
            eb_minibatch_gather(data.* -> update.mb.*)                     six tensors, one launch           (1 kernel)
            update.step()                                                  the PPOUpdate chain               (13 kernels)
            eb_ppo_log(update.rows.*, update.mb.logp_old -> log[e, k])                                       (1 kernel)
        eb_epoch_advance(counter, epochs)                                                                    (1 kernel)

    3 + 15 * epochs * minibatches kernels with normalize.  Minibatch k of epoch e takes the slots k * rows .. (k + 1) * rows - 1 of
    permutation `counter + e` of the N rows of `data` under `seed` (`index_reference(N, seed, e, counter)`), or of perm[e] when an
    [epochs, N] int32 / int64 device tensor is given.  The slots beyond minibatches * rows are dropped.
    `data`: dict of float32 device tensors obs [N, D], actions [N, A], logp_old, adv, ret, v_old [N]; they are read in place at every
    step() / replay, so the caller refills them between iterations.  Everything else is allocated here, once: `counter` (int64, zero),
    the statistics' partials, `log_blocks` [epochs, minibatches, 64, 8] float64 and, with keep_index, `index` [epochs, minibatches, rows]
    int32 (the source row of every destination row).  step() makes no torch operation, no host read, no allocation and no autograd."""

    def __init__(self, update, data, epochs, minibatches, seed=0, normalize=True, perm=None, eps=1e-8, keep_index=False):
        from .train import PPOUpdate
        if not isinstance(update, PPOUpdate):
            raise TypeError('PPOEpochs drives a train.PPOUpdate, got %s' % type(update).__name__)
        self.update, self.epochs, self.minibatches, self.rows = update, int(epochs), int(minibatches), update.n
        if self.epochs < 1 or self.minibatches < 1:
            raise ValueError('epochs and minibatches must be at least 1')
        dev, mb = update.device, update.mb
        self.device, self.seed, self.normalize = dev, int(seed), bool(normalize)
        missing = [k for k in _FIELDS if k not in data]
        if missing:
            raise ValueError('data lacks %s' % ', '.join(missing))
        self.N = N = int(data['obs'].shape[0])
        if N < self.minibatches * self.rows:
            raise ValueError('data holds %d rows, %d minibatches of %d need %d' % (N, self.minibatches, self.rows, self.minibatches * self.rows))
        shapes = dict(obs=(N, mb.obs.shape[1]), actions=(N, mb.actions.shape[1]), logp_old=(N,), adv=(N,), ret=(N,), v_old=(N,))
        self.data = {k: _f32(data[k], 'data[%r]' % k, shapes[k]) for k in _FIELDS}
        if any(t.device != dev for t in self.data.values()):
            raise ValueError('data must live on the device of the networks')
        if perm is not None:
            if not (isinstance(perm, torch.Tensor) and perm.device == dev and perm.dtype in (torch.int32, torch.int64) and perm.is_contiguous()
                    and tuple(perm.shape) == (self.epochs, N)):
                raise TypeError('perm must be a contiguous int32 or int64 device tensor [epochs, N] = [%d, %d]' % (self.epochs, N))
        self.perm = perm
        self.counter = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.partials = torch.zeros((2 * EB_EPOCH_PARTIALS,), dtype=torch.float64, device=dev)
        self.log_blocks = torch.zeros((self.epochs, self.minibatches, EB_EPOCH_LOG_BLOCKS, EB_EPOCH_LOG_FIELDS), dtype=torch.float64, device=dev)
        self.index = torch.zeros((self.epochs, self.minibatches, self.rows), dtype=torch.int32, device=dev) if keep_index else None
        self.api = epoch_api()
        self._stats = EbAdvStatsArgs(n=N, x=_ptr(self.data['adv']), eps=float(eps), out=_ptr(mb.adv_norm), partials=_ptr(self.partials))
        sources, dests = [self.data[k] for k in _FIELDS], [getattr(mb, k) for k in _FIELDS]
        clip = float(update._ppo_args.clip)                      # the surrogate's own clip, as the kernel holds it (fp32)
        self._gathers, self._logs = [], []
        for e in range(self.epochs):
            for k in range(self.minibatches):
                self._gathers.append(_gather_args(sources, dests, k * self.rows, self.rows, None if perm is None else perm[e], self.seed, e,
                                                  self.counter, None if self.index is None else self.index[e, k]))
                self._logs.append(_log_args(update.rows, mb.logp_old, clip, self.log_blocks[e, k], self.rows))
        self._advance = EbEpochAdvanceArgs(counter=_ptr(self.counter), by=self.epochs)
        self.clip = clip

    def step(self):
        """the whole chain, on the current stream"""
        api, upd = self.api, self.update
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            if self.normalize:
                self._stats.stream = s
                api.check(api.adv_stats(C.byref(self._stats)))
            for g, lg in zip(self._gathers, self._logs):
                g.stream = s
                api.check(api.minibatch_gather(C.byref(g)))
                upd.step()
                lg.stream = s
                api.check(api.ppo_log(C.byref(lg)))
            self._advance.stream = s
            api.check(api.epoch_advance(C.byref(self._advance)))

    def capture(self, keep_graph=False):
        """a torch.cuda.CUDAGraph of one step(): a linear chain on one stream, no fork and no join.  Nothing runs during the capture;
        every replay is one iteration's update phase on whatever `data` holds then.  Replay it with `self.replay(graph)` (see
        PPOUpdate.capture for why a bare graph.replay() is not enough)."""
        import gc
        self.update.policy._sync()
        self.update.value._sync()
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
        """graph.replay() for a graph of capture(), and the host-side bookkeeping of PPOUpdate.replay, once: the versions of both flat
        weight tensors move and `_uploaded` follows.  No host read."""
        upd = self.update
        graph.replay()
        upd.adam.bump()
        for net in (upd.policy, upd.value):
            net._uploaded = net._flat._version

    def log(self):
        """one device-to-host copy of log_blocks -> fold_log's dict, every entry an array [epochs, minibatches]"""
        return fold_log(self.log_blocks.cpu().numpy())


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def _splitmix64(z):
    """splitmix64 on a uint64 array (wrap-around)"""
    z = z + np.uint64(GOLDEN)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def index_reference(n, seed, epoch, base=0, walks=False):
    """The whole permutation of [0, n): out[i] = index(key(seed, epoch, base), n, i) of include/envbuild_epoch.h, int64 [n].
    walks: also the number of passes each slot took."""
    n = int(n)
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError('n must be in 1 .. 2^31 - 1')
    b = max(2, (n - 1).bit_length())
    b += b & 1
    h, mask = np.uint64(b // 2), np.uint64((1 << (b // 2)) - 1)
    with np.errstate(over='ignore'):
        start = np.array([(int(seed) + GOLDEN * ((int(base) + int(epoch)) & _M64)) & _M64], np.uint64)
        key = _splitmix64(start)[0]
        x = np.arange(n, dtype=np.uint64)
        steps = np.zeros(n, np.int64)
        todo = np.arange(n)
        while todo.size:
            v = x[todo]
            L, R = v >> h, v & mask
            for r in range(6):
                F = (_splitmix64(key + np.uint64(GOLDEN) * (np.uint64(r << 32) | R)) >> np.uint64(32)) & mask
                L, R = R, L ^ F
            v = (L << h) | R
            x[todo] = v
            steps[todo] += 1
            todo = todo[v >= np.uint64(n)]
    out = x.astype(np.int64)
    return (out, steps) if walks else out


def _halve(a):
    """x[t] += x[t + w] for w = 128 .. 1 along the last axis of 256 -> the last axis' element 0"""
    a = a.copy()
    w = THREADS // 2
    while w:
        a[..., :w] = a[..., :w] + a[..., w:2 * w]
        w //= 2
    return a[..., 0]


def adv_stats_reference(x, eps=1e-8, dtype=np.float32):
    """eb_adv_stats in NumPy -> (mean, inv, std).  The sums S and Q of the deviations from x[0] are the kernels' in both cases: doubles,
    in the header's chunk and halving order.  dtype float32: the kernel's roundings too — its bits; float64: mean, std and 1 / (std + eps) left in double."""
    x = np.asarray(x).reshape(-1)
    n = x.size
    if n < 2:
        raise ValueError('n must be at least 2')
    chunks = -(-n // CHUNK)
    parts = min(chunks, EB_EPOCH_PARTIALS)
    rounds = -(-chunks // parts)
    with np.errstate(all='ignore'):
        shift = np.float64(x[0])
        padded = np.zeros(rounds * parts * CHUNK, np.float64)            # a missing element adds +0.0 to a sum that starts at +0.0
        padded[:n] = x.astype(np.float64) - shift
        cells = padded.reshape(rounds, parts, CHUNK // THREADS, THREADS)
        s, q = np.zeros((parts, THREADS)), np.zeros((parts, THREADS))
        for r in range(rounds):
            for k in range(CHUNK // THREADS):
                v = cells[r, :, k, :]
                s = s + v
                q = q + v * v
        both = np.zeros((2, THREADS))
        both[0, :parts], both[1, :parts] = _halve(s), _halve(q)
        S, Q = _halve(both)
        nn = np.float64(n)
        v = (Q - S * S / nn) / (nn - 1.0)
        var = np.float64(0.0) if v < 0.0 else v                          # a select: a NaN travels
        if np.dtype(dtype) == np.float64:
            sd = np.sqrt(var)
            return shift + S / nn, 1.0 / (sd + np.float64(eps)), sd
        sd = np.float32(np.sqrt(var))
        return np.float32(shift + S / nn), np.float32(1.0) / (sd + np.float32(eps)), sd


def ppo_log_reference(logp=None, logp_old=None, ratio=None, surr=None, ent=None, vloss=None, clip=0.2):
    """eb_ppo_log in NumPy on float32 arrays [n] (None: not given) -> [64, 8] float64, the kernel's blocks in the kernel's order"""
    given = dict(logp=logp, logp_old=logp_old, ratio=ratio, surr=surr, ent=ent, vloss=vloss)
    given = {k: None if v is None else np.asarray(v, np.float32).reshape(-1) for k, v in given.items()}
    sizes = {v.size for v in given.values() if v is not None}
    if len(sizes) != 1:
        raise ValueError('ppo_log_reference needs at least one input, all of one length')
    n = sizes.pop()
    span = EB_EPOCH_LOG_BLOCKS * THREADS
    rounds = max(1, -(-n // span))
    live = (np.arange(rounds * span) < n).reshape(rounds, EB_EPOCH_LOG_BLOCKS, THREADS)

    def cells(a, fill=0.0):
        out = np.full(rounds * span, fill, np.float64)
        out[:n] = a
        return out.reshape(rounds, EB_EPOCH_LOG_BLOCKS, THREADS)

    def total(c):                                                        # lane by lane in ascending rows, then the halving
        acc = np.zeros((EB_EPOCH_LOG_BLOCKS, THREADS))
        for r in range(rounds):
            acc = acc + c[r]
        return _halve(acc)

    out = np.zeros((EB_EPOCH_LOG_BLOCKS, EB_EPOCH_LOG_FIELDS))
    with np.errstate(all='ignore'):
        bad = np.zeros(n, bool)
        for v in given.values():
            if v is not None:
                bad |= ~np.isfinite(v)
        for at, k in ((0, 'surr'), (1, 'vloss'), (2, 'ent')):
            if given[k] is not None:
                out[:, at] = total(cells(given[k].astype(np.float64)))
        if given['ratio'] is not None:
            dev = np.abs(given['ratio'] - np.float32(1.0))               # fp32
            out[:, 3] = total(cells((dev > np.float32(clip)).astype(np.float64)))
            out[:, 5] = cells(np.where(np.isnan(dev), 0.0, dev.astype(np.float64))).max(axis=(0, 2))
        if given['logp'] is not None and given['logp_old'] is not None:
            out[:, 4] = total(cells((given['logp_old'] - given['logp']).astype(np.float64)))
        out[:, 6] = total(cells(bad.astype(np.float64)))
        out[:, 7] = total(live.astype(np.float64))
    return out
