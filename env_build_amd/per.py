"""Prioritised experience replay on the device (include/envbuild_per.h, env_build_amd/csrc/eb_per.hip): a radix-32 sum tree of doubles over
the slots of `offpolicy.ReplayBuffer`'s ring, a stratified draw in proportion to a per-slot priority whose index never goes through the
host, importance weights on the critic loss and a deterministic write-back of the new TD errors as priorities, as library launches —
`reset`, `set_range`, `set_indexed`, `per_sample`, `weigh` — and the Python that strings them together:

`PrioritizedReplayBuffer(capacity, obs_dim, act_dim, device)`: `offpolicy.ReplayBuffer` plus the leaves, the tree, max_prio and the stamp
scratch; `push` gives the new slots the largest priority seen, `sample_into` draws and gathers, `update_priorities(index, value)`.
`Collector(env, policy, buffer, action_range, seed)`: `offpolicy.Collector`'s three launches per env step plus the range route's.
`SAC(policy, q1, q2, buffer, batch, alpha=, beta0=, beta_step=, eps=, ...)`: `offpolicy.SAC` with the prioritised draw in place of the
uniform one and, behind the critic rows, the weights and the write-back: KERNELS = 42 + 2 + eb_per_set_launches(C, indexed) kernel nodes.
`tree_reference`, `set_reference`, `sample_reference` and `weigh_reference` restate the header's contract in NumPy, in the kernels' own
order: the GPU is held to them bit for bit.

The entries live in env_build_amd/lib/libenvbuild_per.so, a library of its own that is bound here on first use (PER_PROTOTYPES): the other
eight libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from . import offpolicy as _off
from .dynamics_and_models import _stream
from .offpolicy import _dev, _f32, _ptr, sample_word_reference
from .policy_sample import _exp_det, _fmaf, _log_det

__all__ = ['PrioritizedReplayBuffer', 'Collector', 'SAC', 'reset', 'set_range', 'set_indexed', 'per_sample', 'weigh', 'tree_levels',
           'tree_doubles', 'set_launches', 'tree_reference', 'set_reference', 'sample_reference', 'weigh_reference', 'EbPerResetArgs',
           'EbPerSetArgs', 'EbPerSampleArgs', 'EbPerWeighArgs', 'EB_PER_ABI_VERSION', 'EB_PER_RADIX', 'EB_PER_MAX_LEVELS',
           'EB_PER_SMALL_NODES', 'EB_PER_MIN_BLOCKS', 'EB_PER_ROUTE_RANGE', 'EB_PER_ROUTE_INDEXED', 'EB_PER_PRIO_MIN', 'EB_PER_PRIO_MAX',
           'PER_PROTOTYPES', 'per_api']

_P, _I, _F, _U = C.c_void_p, C.c_int32, C.c_float, C.c_uint64
EB_PER_ABI_VERSION = 1
EB_PER_RADIX = 32
EB_PER_MAX_LEVELS = 7
EB_PER_SMALL_NODES = 1024
EB_PER_MIN_BLOCKS = 64
EB_PER_ROUTE_RANGE = 0
EB_PER_ROUTE_INDEXED = 1
EB_PER_PRIO_MIN = 2.0 ** -40
EB_PER_PRIO_MAX = 2.0 ** 40
THREADS = 256                                                  # of every kernel (csrc/eb_per_device.h)
HEADER = 'envbuild_per.h'
_f = np.float32
_QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


class EbPerResetArgs(C.Structure):
    """eb_per_reset_args of include/envbuild_per.h"""
    _fields_ = [('capacity', _I), ('prio', _P), ('tree', _P), ('max_prio', _P), ('stamp', _P), ('stream', _P)]


class EbPerSetArgs(C.Structure):
    """eb_per_set_args"""
    _fields_ = [('capacity', _I), ('route', _I), ('n', _I), ('start', _I), ('prio', _P), ('tree', _P), ('max_prio', _P), ('stamp', _P),
                ('index', _P), ('value', _P), ('stream', _P)]


class EbPerSampleArgs(C.Structure):
    """eb_per_sample_args"""
    _fields_ = [('capacity', _I), ('m', _I), ('prio', _P), ('tree', _P), ('seed', _U), ('draw', _U), ('counter', _P), ('u_in', _P),
                ('index_out', _P), ('prio_out', _P), ('noise_id_out', _P), ('min_partials', _P), ('stream', _P)]


class EbPerWeighArgs(C.Structure):
    """eb_per_weigh_args"""
    _fields_ = [('m', _I), ('index', _P), ('prio', _P), ('min_partials', _P), ('q1', _P), ('q2', _P), ('y', _P), ('counter', _P),
                ('beta', _F), ('beta_step', _F), ('alpha', _F), ('eps', _F), ('g_q1', _P), ('g_q2', _P), ('loss1', _P), ('loss2', _P),
                ('w_out', _P), ('prio_new', _P), ('stream', _P)]


# include/envbuild_per.h: name -> (restype, argtypes) for every symbol the header declares
PER_PROTOTYPES = {
    'eb_per_abi_version': (C.c_int, []),
    'eb_per_last_error': (C.c_char_p, []),
    'eb_per_tree_doubles': (C.c_int64, [_I]),
    'eb_per_set_launches': (C.c_int, [_I, _I]),
    'eb_per_reset': (C.c_int, [C.POINTER(EbPerResetArgs)]),
    'eb_per_set': (C.c_int, [C.POINTER(EbPerSetArgs)]),
    'eb_per_sample': (C.c_int, [C.POINTER(EbPerSampleArgs)]),
    'eb_per_weigh': (C.c_int, [C.POINTER(EbPerWeighArgs)]),
}


class PerApi(object):
    """libenvbuild_per.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in PER_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in PER_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_per_abi_version()
        if v != EB_PER_ABI_VERSION:
            raise _capi.EbError('%s: per ABI version %d, expected %d (include/%s)' % (path, v, EB_PER_ABI_VERSION, HEADER))
        lib = self.lib
        self.reset, self.set, self.sample, self.weigh = lib.eb_per_reset, lib.eb_per_set, lib.eb_per_sample, lib.eb_per_weigh

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_per_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(per): %s' % msg)
            raise _capi.EbError('envbuild(per) error %d: %s' % (rc, msg))


_per_api = None


def per_api():
    """The prioritised-replay library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never
    falls back — when it is absent or was built from other sources and cannot be rebuilt."""
    global _per_api
    if _per_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.per_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.PER_LIB, _build.CSRC))
            try:
                _build.build_per()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.PER_LIB, e))
        _per_api = PerApi(_build.PER_LIB)
    return _per_api


def _issue(fn_name, a, device):
    api = per_api()
    with torch.cuda.device(device):
        a.stream = _stream(device)
        api.check(getattr(api, fn_name)(C.byref(a)))


# ---- the tree's geometry (the header's formula) ---------------------------------------------------------------------------------------------
def tree_levels(capacity):
    """-> (n, off, first_small): n[0] = C and n[k] = ceil(n[k - 1] / 32) up to the level with one node; off[k] the level's place in the
    tree array (off[0] is None, level 1 first, the root last); first_small: the lowest level with at most 1024 nodes"""
    C_ = int(capacity)
    if not 1 <= C_ <= 2 ** 31 - 1:
        raise ValueError('capacity must be in 1 .. 2^31 - 1, got %d' % C_)
    n, off, at = [C_], [None], 0
    while True:
        n.append(-(-n[-1] // EB_PER_RADIX))
        off.append(at)
        at += n[-1]
        if n[-1] == 1:
            break
    first_small = len(n) - 1
    while first_small > 1 and n[first_small - 1] <= EB_PER_SMALL_NODES:
        first_small -= 1
    return n, off, first_small


def tree_doubles(capacity):
    """eb_per_tree_doubles in Python: the tree array's length"""
    n, _, _ = tree_levels(capacity)
    return sum(n[1:])


def set_launches(capacity, route):
    """eb_per_set_launches in Python: big(C) + 2 on the range route, big(C) + 3 on the indexed one"""
    _, _, first_small = tree_levels(capacity)
    if route not in (EB_PER_ROUTE_RANGE, EB_PER_ROUTE_INDEXED):
        raise ValueError('route must be EB_PER_ROUTE_RANGE or EB_PER_ROUTE_INDEXED')
    return first_small - 1 + (2 if route == EB_PER_ROUTE_RANGE else 3)


# ---- the contract in NumPy --------------------------------------------------------------------------------------------------------------------
def _level_up(children):
    """the sums of consecutive groups of 32 doubles, each ascending from 0.0, one double addition per existing child"""
    k = len(children)
    groups = -(-k // EB_PER_RADIX)
    padded = np.zeros(groups * EB_PER_RADIX, np.float64)
    padded[:k] = children
    padded = padded.reshape(groups, EB_PER_RADIX)
    s = np.zeros(groups, np.float64)
    for c in range(EB_PER_RADIX):
        s = s + padded[:, c]                                      # (x + 0.0 == x for the non-negative sums: a missing child adds nothing)
    return s


def tree_reference(prio):
    """the full build: prio [C] float32 -> the tree array (float64 [tree_doubles(C)]), level 1 first, the root last"""
    prio = np.asarray(prio, _f).reshape(-1)
    n, off, _ = tree_levels(len(prio))
    tree = np.zeros(sum(n[1:]), np.float64)
    level = prio.astype(np.float64)
    for k in range(1, len(n)):
        level = _level_up(level)
        assert len(level) == n[k]
        tree[off[k]:off[k] + n[k]] = level
    return tree


def _valid_rows(index, value, capacity):
    with np.errstate(invalid='ignore'):
        return (index >= 0) & (index < capacity) & (value > 0) & (value < np.inf)


def set_reference(prio, max_prio, start=None, n=None, index=None, value=None):
    """eb_per_set on NumPy arrays -> (prio, max_prio), new arrays; the tree is tree_reference(prio).  Range route: start, n.  Indexed route:
    index [m] and value [m]; the highest valid row of a leaf wins (NumPy's own order of prio[index[valid]] = value[valid])."""
    prio = np.asarray(prio, _f).copy()
    max_prio = _f(max_prio)
    C_ = len(prio)
    if index is None:
        prio[(int(start) + np.arange(int(n), dtype=np.int64)) % C_] = max_prio
        return prio, max_prio
    index, value = np.asarray(index, np.int64).reshape(-1), np.asarray(value, _f).reshape(-1)
    ok = _valid_rows(index, value, C_)
    stored = np.minimum(np.maximum(value[ok], _f(EB_PER_PRIO_MIN)), _f(EB_PER_PRIO_MAX)).astype(_f)
    for j, v in zip(index[ok], stored):                           # ascending rows: the last writer of a leaf is its highest row
        prio[j] = v
    if len(stored):
        max_prio = max(max_prio, stored.max())
    return prio, _f(max_prio)


def _scan(children, exists, u):
    """the descent's step at one node per row: children [m, 32] float64 (0.0 where none exists), u [m] -> (chosen [m], u' [m])"""
    m = len(u)
    acc, base = np.zeros(m, np.float64), np.zeros(m, np.float64)
    chosen, last = np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    for c in range(EB_PER_RADIX):
        s = children[:, c]
        nxt = acc + s
        hit = (chosen < 0) & exists[:, c] & (u < nxt)
        chosen = np.where(hit, c, chosen)
        base = np.where(hit, acc, base)
        last = np.where(s > 0, c, last)
        acc = nxt
    none = chosen < 0
    return np.where(none, last, chosen), np.where(none, 0.0, u - base)


def sample_reference(prio, m, seed=0, draw=0, base=0, u_in=None, tree=None):
    """eb_per_sample on NumPy arrays -> dict(index int32 [m], prio float32 [m], noise_id uint32 [m], min_partials float32 [64]).  tree: the
    tree array to descend (default: tree_reference(prio); a hand-made one reaches the fallback)."""
    prio = np.asarray(prio, _f).reshape(-1)
    m = int(m)
    n, off, _ = tree_levels(len(prio))
    tree = tree_reference(prio) if tree is None else np.asarray(tree, np.float64)
    word = sample_word_reference(m, seed, draw, base)
    total = tree[-1]
    U = (word >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 if u_in is None else np.asarray(u_in, np.float64).reshape(m)
    rows = np.arange(m, dtype=np.float64)
    with np.errstate(all='ignore'):
        u = (rows + U) * (total / np.float64(m))
    node = np.zeros(m, np.int64)
    alive = np.full(m, bool(total > 0))
    for k in range(len(n) - 1, 0, -1):
        level = prio.astype(np.float64) if k == 1 else tree[off[k - 1]:off[k - 1] + n[k - 1]]
        at = np.where(alive, node, 0)[:, None] * EB_PER_RADIX + np.arange(EB_PER_RADIX)
        exists = at < n[k - 1]
        children = np.where(exists, level[np.minimum(at, n[k - 1] - 1)], 0.0)
        c, u = _scan(children, exists, u)
        alive &= c >= 0
        node = np.where(alive, node * EB_PER_RADIX + c, -1)
    index = np.where(alive, node, -1).astype(np.int32)
    drawn = np.where(alive, prio[np.where(alive, node, 0)], _QNAN).astype(_f)
    partials = np.full(EB_PER_MIN_BLOCKS, np.inf, _f)
    block = (np.arange(m) // THREADS) % EB_PER_MIN_BLOCKS
    for b in np.unique(block[alive]):
        partials[b] = drawn[alive & (block == b)].min()
    return dict(index=index, prio=drawn, noise_id=(word & np.uint64(0xFFFFFFFF)).astype(np.uint32), min_partials=partials)


def beta_reference(beta, beta_step=0.0, counter=None):
    """eb_per_weigh's beta: by value, or min(1, fmaf(beta_step, (float)counter, beta))"""
    if counter is None:
        return _f(beta)
    b = _fmaf(_f(beta_step), np.asarray(np.uint64(counter)).astype(_f), _f(beta)).reshape(())
    return _f(b) if b < 1 else _f(1)


def weigh_reference(index, prio, min_partials, q1=None, q2=None, y=None, beta=0.4, beta_step=0.0, counter=None, alpha=0.6, eps=1e-6,
                    g_q1=None, g_q2=None, loss1=None, loss2=None):
    """eb_per_weigh in NumPy, one fp32 rounding per line -> dict(w, prio_new (with q1 and y), and g_q1, g_q2, loss1, loss2 scaled, each
    when given)"""
    index, prio = np.asarray(index, np.int64).reshape(-1), np.asarray(prio, _f).reshape(-1)
    drawn = index >= 0
    with np.errstate(all='ignore'):
        b = beta_reference(beta, beta_step, counter)
        p_min = np.asarray(min_partials, _f).min()
        d = _log_det(np.full(len(prio), p_min, _f)) - _log_det(prio)
        w = np.where(drawn, _exp_det((b * d).astype(_f)), _f(0)).astype(_f)
        out = dict(w=w)
        for name, g in (('g_q1', g_q1), ('g_q2', g_q2), ('loss1', loss1), ('loss2', loss2)):
            if g is not None:
                out[name] = (np.asarray(g, _f).reshape(-1) * w).astype(_f)
        if q1 is not None and y is not None:
            q1, y = np.asarray(q1, _f).reshape(-1), np.asarray(y, _f).reshape(-1)
            a = np.abs(q1 - y)
            if q2 is not None:
                a = _f(0.5) * (a + np.abs(np.asarray(q2, _f).reshape(-1) - y))
            s = (a + _f(eps)).astype(_f)
            new = s if _f(alpha) == _f(1) else _exp_det((_f(alpha) * _log_det(s)).astype(_f))
            out['prio_new'] = np.where(drawn, new, _QNAN).astype(_f)
    return out


# ---- the entries --------------------------------------------------------------------------------------------------------------------------------
def _i32(t, what, shape, device):
    return None if t is None else _dev(t, what, np.int32, shape, device)


def reset(buffer):
    """eb_per_reset on a PrioritizedReplayBuffer: ONE launch"""
    _issue('reset', buffer.reset_args(), buffer.device)


def set_range(buffer, start, n):
    """eb_per_set, range route: the slots (start + i) mod C, i < n, take *max_prio; the tree is repaired"""
    _issue('set', buffer.set_args(EB_PER_ROUTE_RANGE, n, start=start), buffer.device)


def set_indexed(buffer, index, value):
    """eb_per_set, indexed route: prio[index[valid]] = clamp(value[valid]), the highest row of a leaf wins; the tree is repaired"""
    _issue('set', buffer.set_args(EB_PER_ROUTE_INDEXED, index.numel(), index=index, value=value), buffer.device)


def per_sample(buffer, index, prio=None, noise_id=None, min_partials=None, seed=0, draw=0, counter=None, u_in=None):
    """eb_per_sample: index.numel() stratified draws in proportion to the leaves.  ONE launch."""
    _issue('sample', buffer.draw_args(index, prio, noise_id, min_partials, seed, draw, counter, u_in), buffer.device)


def _weigh_args(index, prio, min_partials, q1=None, q2=None, y=None, beta=0.4, beta_step=0.0, counter=None, alpha=0.6, eps=1e-6,
                g_q1=None, g_q2=None, loss1=None, loss2=None, w_out=None, prio_new=None):
    m, dev = index.numel(), index.device
    _i32(index, 'index', (m,), dev), _f32(min_partials, 'min_partials', (EB_PER_MIN_BLOCKS,), dev)
    for name, t in (('prio', prio), ('q1', q1), ('q2', q2), ('y', y), ('g_q1', g_q1), ('g_q2', g_q2), ('loss1', loss1), ('loss2', loss2),
                    ('w_out', w_out), ('prio_new', prio_new)):
        if t is not None and _dev(t, name, device=dev).numel() != m:
            raise ValueError('%s must hold %d values' % (name, m))
    if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise TypeError('counter must be a device int64 tensor of one element')
    return EbPerWeighArgs(m=m, index=_ptr(index), prio=_ptr(prio), min_partials=_ptr(min_partials), q1=_ptr(q1), q2=_ptr(q2), y=_ptr(y),
                          counter=_ptr(counter), beta=float(beta), beta_step=float(beta_step), alpha=float(alpha), eps=float(eps),
                          g_q1=_ptr(g_q1), g_q2=_ptr(g_q2), loss1=_ptr(loss1), loss2=_ptr(loss2), w_out=_ptr(w_out), prio_new=_ptr(prio_new))


def weigh(index, prio, min_partials, **kw):
    """eb_per_weigh: the importance weights (g_q1, g_q2, loss1, loss2 scaled in place; w_out) and the new priorities (prio_new, from q1,
    q2 or None, y).  Keywords: beta (| beta_step and counter), alpha, eps.  ONE launch."""
    _issue('weigh', _weigh_args(index, prio, min_partials, **kw), index.device)


# ---- the buffer ---------------------------------------------------------------------------------------------------------------------------------
class PrioritizedReplayBuffer(_off.ReplayBuffer):
    """`offpolicy.ReplayBuffer` with the structure of include/envbuild_per.h on the device: prio [C] float32, tree [tree_doubles(C)]
    float64, max_prio [1] and stamp [C] int32.  push() is the parent's push plus the range route over the slots it wrote; sample_into()
    draws in proportion to the leaves (eb_per_sample) and gathers the rows with the parent's eb_replay_sample; update_priorities()
    is the indexed route.  The invariant holds after each of them."""

    def __init__(self, capacity, obs_dim, act_dim, device=None):
        super(PrioritizedReplayBuffer, self).__init__(capacity, obs_dim, act_dim, device)
        dev, C_ = self.device, self.capacity
        self.prio = torch.zeros((C_,), dtype=torch.float32, device=dev)
        self.tree = torch.zeros((tree_doubles(C_),), dtype=torch.float64, device=dev)
        self.max_prio = torch.ones((1,), dtype=torch.float32, device=dev)
        self.stamp = torch.full((C_,), -1, dtype=torch.int32, device=dev)
        self.api = per_api()
        if self.api.lib.eb_per_tree_doubles(C_) != self.tree.numel():
            raise _capi.EbError('eb_per_tree_doubles(%d) disagrees with per.tree_doubles' % C_)
        reset(self)

    def reset_args(self):
        return EbPerResetArgs(capacity=self.capacity, prio=_ptr(self.prio), tree=_ptr(self.tree), max_prio=_ptr(self.max_prio),
                              stamp=_ptr(self.stamp))

    def set_args(self, route, n, start=0, index=None, value=None):
        """eb_per_set_args over this buffer's structure"""
        n = int(n)
        if route == EB_PER_ROUTE_INDEXED and n:
            _i32(index, 'index', (n,), self.device), _f32(value, 'value', (n,), self.device)
        return EbPerSetArgs(capacity=self.capacity, route=route, n=n, start=int(start), prio=_ptr(self.prio), tree=_ptr(self.tree),
                            max_prio=_ptr(self.max_prio), stamp=_ptr(self.stamp), index=_ptr(index), value=_ptr(value))

    def draw_args(self, index, prio=None, noise_id=None, min_partials=None, seed=0, draw=0, counter=None, u_in=None):
        """eb_per_sample_args over this buffer's structure"""
        m, dev = index.numel(), self.device
        _i32(index, 'index', (m,), dev), _f32(prio, 'prio', (m,), dev), _i32(noise_id, 'noise_id', (m,), dev)
        _f32(min_partials, 'min_partials', (EB_PER_MIN_BLOCKS,), dev)
        if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
            raise TypeError('counter must be a device int64 tensor of one element')
        if u_in is not None:
            _dev(u_in, 'u_in', np.float64, (m,), dev)
        return EbPerSampleArgs(capacity=self.capacity, m=m, prio=_ptr(self.prio), tree=_ptr(self.tree), seed=int(seed) & (2 ** 64 - 1),
                               draw=int(draw) & (2 ** 64 - 1), counter=_ptr(counter), u_in=_ptr(u_in), index_out=_ptr(index),
                               prio_out=_ptr(prio), noise_id_out=_ptr(noise_id), min_partials=_ptr(min_partials))

    def launches(self, route):
        """eb_per_set_launches(C, route), from the library"""
        return int(self.api.lib.eb_per_set_launches(self.capacity, route))

    def push(self, prev_obs, action, reward, obs_after, done_code, final_obs=None):
        """the parent's push (ONE launch) and the range route over the slots it wrote: they take *max_prio"""
        start, n = self.cursor, reward.numel()
        super(PrioritizedReplayBuffer, self).push(prev_obs, action, reward, obs_after, done_code, final_obs)
        set_range(self, start, n)

    def gather_args(self, batch, seed=0, draw=0, counter=None):
        """the parent's eb_replay_sample_args with indices = batch's index (the draw's output), which is not written again"""
        get = batch.get if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        rows = {k: get(k) for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal') if get(k) is not None}
        return self.sample_args(rows, seed, draw, counter, indices=get('index'))

    def sample_into(self, batch, seed=0, draw=0, counter=None, u_in=None):
        """eb_per_sample into batch's index (needed), prio and min_partials (each optional), then eb_replay_sample with those indices into
        the rest of `batch` (as the parent's sample_into): TWO launches on the current stream."""
        get = batch.get if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        if get('index') is None:
            raise ValueError('a prioritised sample needs batch["index"] (int32 [m])')
        per_sample(self, get('index'), get('prio'), get('noise_id'), get('min_partials'), seed, draw, counter, u_in)
        if any(get(k) is not None for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal')):
            _off._issue('sample', self.gather_args(batch, seed, draw, counter), self.device)

    def update_priorities(self, index, value):
        """eb_per_set, indexed route: index int32 [m] (a draw's output) and value float32 [m] (eb_per_weigh's prio_new) on the device"""
        set_indexed(self, index, value)

    def structure(self):
        """prio, tree, max_prio and stamp as NumPy copies"""
        return {k: getattr(self, k).cpu().numpy().copy() for k in ('prio', 'tree', 'max_prio', 'stamp')}


# ---- the collector ------------------------------------------------------------------------------------------------------------------------------
class Collector(_off.Collector):
    """`offpolicy.Collector` into a PrioritizedReplayBuffer: its three launches per env step, then the range route's
    eb_per_set_launches(C, range) over the slots the step wrote."""

    def __init__(self, env, policy, buffer, action_range, seed=0):
        if not isinstance(buffer, PrioritizedReplayBuffer):
            raise TypeError('per.Collector fills a PrioritizedReplayBuffer, got %s' % type(buffer).__name__)
        super(Collector, self).__init__(env, policy, buffer, action_range, seed)
        self._set = buffer.set_args(EB_PER_ROUTE_RANGE, self.n_env)

    def _step(self, random):
        start = self.buffer.cursor
        super(Collector, self)._step(random)
        with torch.cuda.device(self.device):
            self._set.start, self._set.stream = start, _stream(self.device)
            self.buffer.api.check(self.buffer.api.set(C.byref(self._set)))


# ---- one prioritised SAC update -----------------------------------------------------------------------------------------------------------------
class SAC(_off.SAC):
    """`offpolicy.SAC` on a PrioritizedReplayBuffer.  The chain is the parent's, restated nowhere; two of its pieces are replaced:

         1  eb_per_sample               mb.index, mb.prio, mb.noise_id, min_partials: `batch` stratified draws in proportion to the leaves   (1)
            eb_replay_sample            the parent's gather, indices = mb.index                                                            (1)
        ...
         4  eb_sac_critic               as the parent's                                                                                    (1)
            eb_per_weigh                w; g_q1, g_q2, loss1, loss2 scaled in place; prio_new from the step's own q1, q2, y                (1)
            eb_per_set (indexed)        the leaves at mb.index take prio_new, the tree is repaired             (eb_per_set_launches(C, indexed))
        ...

    beta = min(1, beta0 + beta_step * the draw counter) is formed on the device, so a replayed graph anneals it.  KERNELS — the kernel
    nodes of capture()'s graph — is 42 + 2 + eb_per_set_launches(C, indexed) and depends on the buffer's capacity: an instance attribute.
    `eps` is the priority's (prio_new = (|TD| + eps)^alpha); Adam's is `adam_eps`."""

    def __init__(self, policy, q1, q2, buffer, batch, alpha=0.6, beta0=0.4, beta_step=0.0, eps=1e-6, adam_eps=1e-8, **kw):
        if not isinstance(buffer, PrioritizedReplayBuffer):
            raise TypeError('per.SAC draws from a PrioritizedReplayBuffer, got %s' % type(buffer).__name__)
        for name, v in (('alpha', alpha), ('beta0', beta0), ('beta_step', beta_step), ('eps', eps)):
            if not np.isfinite(v):
                raise ValueError('%s must be finite, got %r' % (name, v))
        super(SAC, self).__init__(policy, q1, q2, buffer, batch, eps=adam_eps, **kw)                  # (the parent's eps is Adam's)
        n, dev, r, mb = self.n, self.device, self.rows, self.mb
        self.per_alpha, self.beta0, self.beta_step, self.per_eps = float(alpha), float(beta0), float(beta_step), float(eps)
        mb.index = torch.zeros((n,), dtype=torch.int32, device=dev)
        mb.prio = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.min_partials = torch.zeros((EB_PER_MIN_BLOCKS,), dtype=torch.float32, device=dev)
        r.w, r.prio_new = torch.zeros((n,), dtype=torch.float32, device=dev), torch.zeros((n,), dtype=torch.float32, device=dev)
        self.per = buffer.api
        self._a_draw = buffer.draw_args(mb.index, mb.prio, mb.noise_id, self.min_partials, seed=self.seed, draw=0, counter=self.counter)
        self._a_sample = buffer.gather_args(mb, seed=self.seed, draw=0, counter=self.counter)
        self._a_weigh = _weigh_args(mb.index, mb.prio, self.min_partials, q1=r.q1, q2=r.q2, y=r.y, beta=self.beta0, beta_step=self.beta_step,
                                    counter=self.counter, alpha=self.per_alpha, eps=self.per_eps, g_q1=r.g_q1, g_q2=r.g_q2, loss1=r.loss1,
                                    loss2=r.loss2, w_out=r.w, prio_new=r.prio_new)
        self._a_set = buffer.set_args(EB_PER_ROUTE_INDEXED, n, index=mb.index, value=r.prio_new)
        self.KERNELS = _off.SAC.KERNELS + 2 + buffer.launches(EB_PER_ROUTE_INDEXED)
        self._log_per = torch.zeros((n,), dtype=torch.float32, device=dev)

    def _draw(self, s):
        self._a_draw.stream = s
        self.per.check(self.per.sample(C.byref(self._a_draw)))
        super(SAC, self)._draw(s)

    def _after_critic(self, s):
        self._a_weigh.stream = self._a_set.stream = s
        self.per.check(self.per.weigh(C.byref(self._a_weigh)))
        self.per.check(self.per.set(C.byref(self._a_set)))

    def log(self):
        """the parent's log (the critic losses are the weighted ones) plus `weight`, the mean importance weight of the last update, and
        `beta`, the one it used"""
        out = super(SAC, self).log()
        self._log_per.copy_(self.rows.w)
        counter = int(self.counter.item()) - 1                    # the update advanced it
        out['weight'] = float(self._log_per.cpu().numpy().astype(np.float64).mean())
        out['beta'] = float(beta_reference(self.beta0, self.beta_step, max(counter, 0)))
        return out
