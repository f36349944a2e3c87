"""Running observation and reward normalisation on the device (include/envbuild_norm.h, env_build_amd/csrc/eb_norm.hip): the reference's
'normalize' preprocessor (utils/preprocessor.py: RunningMeanStd, process_obs, process_rew, np_process_obses, np_process_rewards) as
library launches — a batch merged into the running statistics with TWO launches (`update`), the normalisation with ONE (`apply`) — the
statistics living in device memory from the first batch to the last, and `Collector`, which strings the two into
`collect.Collector`'s loop: three more launches per env step, no torch operation, no allocation, no host read.

`NormState(D, device, epsilon)`: the state of width D — stat (float64 [2 D + 1]: mean, var, count) and scale (float32 [2 D]: mean_f,
den_f) on the device — with get_params / set_params / save_params / load_params (an .npz, or the reference's ppc_params.npy dict).
`update(obs_state, x, ret_state, reward, ret_run, gamma)`: eb_norm_update.  `apply(obs_state, x, out, ...)`: eb_norm_apply.
`HostState`, `update_reference`, `update_return_reference`, `apply_reference` and `apply_reward_reference` restate the header's contract
in NumPy, in the kernels' own order: the GPU is held to them bit for bit.  `Preprocessor` has the reference's constructor and method
names over the device state.

The entries live in env_build_amd/lib/libenvbuild_norm.so, a library of its own that is bound here on first use (NORM_PROTOTYPES): the
other six libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from . import collect as _collect
from .dynamics_and_models import _stream, _unwrap

__all__ = ['NormState', 'HostState', 'update', 'apply', 'update_reference', 'update_return_reference', 'apply_reference',
           'apply_reward_reference', 'partial_sums_reference', 'Preprocessor', 'Collector', 'EbNormUpdateArgs', 'EbNormApplyArgs',
           'EB_NORM_ABI_VERSION', 'EB_NORM_MAX_DIM', 'EB_NORM_MAX_BLOCKS', 'NORM_PROTOTYPES', 'norm_api', 'workspace_bytes']

_P, _I, _F = C.c_void_p, C.c_int32, C.c_float
EB_NORM_ABI_VERSION = 1
EB_NORM_MAX_DIM = 256
EB_NORM_MAX_BLOCKS = 512
THREADS = 256                                                  # of every kernel (csrc/eb_norm_device.h)
ROWS = 32                                                      # rows of one run
INITIAL_COUNT = 1e-4                                           # RunningMeanStd(epsilon=1e-4): preprocessor.py:29-32
HEADER = 'envbuild_norm.h'


class EbNormUpdateArgs(C.Structure):
    """eb_norm_update_args of include/envbuild_norm.h"""
    _fields_ = [('n', _I), ('dim', _I), ('x', _P), ('obs_stat', _P), ('obs_scale', _P), ('reward', _P), ('ret_run', _P), ('ret_stat', _P),
                ('ret_scale', _P), ('workspace', _P), ('gamma', _F), ('eps', _F), ('stream', _P)]


class EbNormApplyArgs(C.Structure):
    """eb_norm_apply_args"""
    _fields_ = [('n', _I), ('dim', _I), ('obs_scale', _P), ('x', _P), ('y', _P), ('sel_x', _P), ('sel', _P), ('sel_value', _I),
                ('clip_obs', _F), ('ret_scale', _P), ('reward', _P), ('reward_out', _P), ('done_code', _P), ('ret_run', _P),
                ('clip_rew', _F), ('stream', _P)]


# include/envbuild_norm.h: name -> (restype, argtypes) for every symbol the header declares
NORM_PROTOTYPES = {
    'eb_norm_abi_version': (C.c_int, []),
    'eb_norm_last_error': (C.c_char_p, []),
    'eb_norm_workspace_bytes': (C.c_size_t, [C.c_int32]),
    'eb_norm_update': (C.c_int, [C.POINTER(EbNormUpdateArgs)]),
    'eb_norm_apply': (C.c_int, [C.POINTER(EbNormApplyArgs)]),
}


class NormApi(object):
    """libenvbuild_norm.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in NORM_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in NORM_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_norm_abi_version()
        if v != EB_NORM_ABI_VERSION:
            raise _capi.EbError('%s: norm ABI version %d, expected %d (include/%s)' % (path, v, EB_NORM_ABI_VERSION, HEADER))
        self.update, self.apply, self.workspace_bytes = self.lib.eb_norm_update, self.lib.eb_norm_apply, self.lib.eb_norm_workspace_bytes

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_norm_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(norm): %s' % msg)
            raise _capi.EbError('envbuild(norm) error %d: %s' % (rc, msg))


_norm_api = None


def norm_api():
    """The normalisation library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls
    back — when it is absent or was built from other sources and cannot be rebuilt."""
    global _norm_api
    if _norm_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.norm_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.NORM_LIB, _build.CSRC))
            try:
                _build.build_norm()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.NORM_LIB, e))
        _norm_api = NormApi(_build.NORM_LIB)
    return _norm_api


def workspace_bytes(D):
    """eb_norm_workspace_bytes restated: EB_NORM_MAX_BLOCKS * 2 * (D + 1) doubles"""
    D = int(D)
    return EB_NORM_MAX_BLOCKS * 2 * (D + 1) * 8 if 1 <= D <= EB_NORM_MAX_DIM else 0


def _ptr(t):
    return None if t is None else t.data_ptr()


_dev = _collect._dev


def _width(D):
    D = int(D)
    if not 1 <= D <= EB_NORM_MAX_DIM:
        raise ValueError('the width must be in 1 .. %d, got %d' % (EB_NORM_MAX_DIM, D))
    return D


# ---- the state ------------------------------------------------------------------------------------------------------------------------------
def _scale_of(mean, var, eps_f):
    """mean_f = (float)mean, den_f = sqrtf((float)var + eps_f): the header's two formulas -> float32 [2 D]"""
    with np.errstate(all='ignore'):
        mean_f = np.asarray(mean, np.float64).astype(np.float32)
        den_f = np.sqrt(np.asarray(var, np.float64).astype(np.float32) + np.float32(eps_f)).astype(np.float32)
    return np.concatenate([mean_f.reshape(-1), den_f.reshape(-1)])


def _params(D, mean, var, count):
    mean = np.broadcast_to(np.asarray(mean, np.float64).reshape(-1), (D,)) if np.size(mean) in (1, D) else None
    var = np.broadcast_to(np.asarray(var, np.float64).reshape(-1), (D,)) if np.size(var) in (1, D) else None
    if mean is None or var is None:
        raise ValueError('mean and var must hold %d values' % D)
    return np.concatenate([mean, var, [np.float64(count)]])


class HostState(object):
    """the state of width D in NumPy, what the restatements work on: stat float64 [2 D + 1] (mean, var, count), scale float32 [2 D]
    (mean_f, den_f), eps_f (the fp32 rounding of epsilon).  Initially the reference's: mean 0, var 1, count 1e-4."""

    def __init__(self, D, epsilon=1e-8):
        self.D, self.epsilon, self.eps_f = _width(D), float(epsilon), np.float32(epsilon)
        if not np.isfinite(self.eps_f):
            raise ValueError('epsilon must be finite, got %r' % (epsilon,))
        self.set_params(0.0, 1.0, INITIAL_COUNT)

    def get_params(self):
        D = self.D
        return self.stat[:D].copy(), self.stat[D:2 * D].copy(), float(self.stat[2 * D])

    def set_params(self, mean, var, count):
        self.stat = _params(self.D, mean, var, count)
        self.scale = _scale_of(self.stat[:self.D], self.stat[self.D:2 * self.D], self.eps_f)

    def copy(self):
        out = HostState(self.D, self.epsilon)
        out.stat, out.scale = self.stat.copy(), self.scale.copy()
        return out


def _read_params(path):
    """(mean, var, count) per key ('ob_rms', 'ret_rms') from an .npz of this module or the reference's ppc_params.npy dict"""
    if str(path).endswith('.npy'):
        params = np.load(path, allow_pickle=True).item()                 # preprocessor.py:176-182: np.save of get_params()'s dict
        return {k: tuple(v) for k, v in params.items()}
    z = np.load(path)
    return {k: (z[k + '_mean'], z[k + '_var'], float(z[k + '_count'])) for k in ('ob_rms', 'ret_rms') if k + '_mean' in z}


class NormState(object):
    """the state of width D on the device — `stat` (float64 [2 D + 1]) and `scale` (float32 [2 D]) — and the workspace eb_norm_update
    needs for it.  Parameters are set from the host with the same IEEE operations the kernel uses (HostState)."""

    def __init__(self, D, device, epsilon=1e-8):
        from .dynamics_and_models import _resolve_device
        self.D, self.device, self.epsilon, self.eps_f = _width(D), _resolve_device(device), float(epsilon), np.float32(epsilon)
        self.stat = torch.zeros((2 * self.D + 1,), dtype=torch.float64, device=self.device)
        self.scale = torch.zeros((2 * self.D,), dtype=torch.float32, device=self.device)
        self.work = torch.zeros((workspace_bytes(self.D) // 8,), dtype=torch.float64, device=self.device)
        self.set_params(0.0, 1.0, INITIAL_COUNT)

    def host(self):
        """a HostState with this state's bits"""
        out = HostState(self.D, self.epsilon)
        out.stat, out.scale = self.stat.cpu().numpy().copy(), self.scale.cpu().numpy().copy()
        return out

    def get_params(self):
        """(mean [D], var [D], count) as float64"""
        return self.host().get_params()

    def set_params(self, mean, var, count):
        h = HostState(self.D, self.epsilon)
        h.set_params(mean, var, count)
        self.stat.copy_(torch.from_numpy(h.stat))
        self.scale.copy_(torch.from_numpy(h.scale))

    def save_params(self, path, key='ob_rms'):
        mean, var, count = self.get_params()
        np.savez(path, **{key + '_mean': mean, key + '_var': var, key + '_count': np.float64(count)})

    def load_params(self, path, key='ob_rms'):
        self.set_params(*_read_params(path)[key])


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def _update_args(obs_state=None, x=None, ret_state=None, reward=None, ret_run=None, gamma=0.99):
    """eb_norm_update_args; x / reward may be set later (their pointers alone change from step to step)"""
    if obs_state is None and ret_state is None:
        raise ValueError('update needs an observation state, a return state or both')
    own = obs_state if obs_state is not None else ret_state
    a = EbNormUpdateArgs(dim=own.D, workspace=_ptr(own.work), gamma=float(gamma), eps=float(own.eps_f))
    n = None
    if obs_state is not None:
        a.obs_stat, a.obs_scale = _ptr(obs_state.stat), _ptr(obs_state.scale)
        if x is not None:
            _dev(x, 'x', device=obs_state.device)
            if x.dim() != 2 or x.shape[1] != obs_state.D:
                raise ValueError('x must be [n, %d], got %s' % (obs_state.D, tuple(x.shape)))
            a.x, n = _ptr(x), x.shape[0]
    if ret_state is not None:
        if ret_state.D != 1:
            raise ValueError('the return state has width 1, got %d' % ret_state.D)
        if obs_state is not None and ret_state.eps_f != obs_state.eps_f:
            raise ValueError('the two states of one update share their epsilon')
        a.ret_stat, a.ret_scale = _ptr(ret_state.stat), _ptr(ret_state.scale)
        if reward is not None:
            m = reward.numel()
            if n is not None and m != n:
                raise ValueError('reward must hold %d values, got %d' % (n, m))
            _dev(reward, 'reward', device=ret_state.device)
            _dev(ret_run, 'ret_run', np.float32, (m,), ret_state.device)
            a.reward, a.ret_run, n = _ptr(reward), _ptr(ret_run), m
    a.n = 0 if n is None else n
    return a


def update(obs_state=None, x=None, ret_state=None, reward=None, ret_run=None, gamma=0.99):
    """eb_norm_update: x [n, D] merged into `obs_state`, and / or R = ret_run * gamma + reward (written back to ret_run [n]) merged into
    `ret_state` (width 1).  TWO launches on the current stream."""
    a = _update_args(obs_state, x, ret_state, reward, ret_run, gamma)
    api, dev = norm_api(), (obs_state if obs_state is not None else ret_state).device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.update(C.byref(a)))


def _apply_args(obs_state=None, x=None, out=None, clip=10., sel_x=None, sel=None, sel_value=0, ret_state=None, reward=None, reward_out=None,
                done_code=None, ret_run=None, clip_rew=10.):
    a = EbNormApplyArgs(dim=1 if obs_state is None else obs_state.D, sel_value=int(sel_value), clip_obs=float(clip), clip_rew=float(clip_rew))
    n = None
    if obs_state is not None:
        a.obs_scale = _ptr(obs_state.scale)
        if x is not None:
            _dev(x, 'x', device=obs_state.device)
            if x.dim() != 2 or x.shape[1] != obs_state.D:
                raise ValueError('x must be [n, %d], got %s' % (obs_state.D, tuple(x.shape)))
            out = x if out is None else _dev(out, 'out', np.float32, tuple(x.shape), obs_state.device)
            a.x, a.y, n = _ptr(x), _ptr(out), x.shape[0]
        if sel_x is not None:
            _dev(sel_x, 'sel_x', device=obs_state.device)
            if sel_x.dim() != 2 or sel_x.shape[1] != obs_state.D or (n is not None and sel_x.shape[0] != n):
                raise ValueError('sel_x must be [n, %d], got %s' % (obs_state.D, tuple(sel_x.shape)))
            n = sel_x.shape[0]
            _dev(sel, 'sel', np.int32, (n,), obs_state.device)
            a.sel_x, a.sel = _ptr(sel_x), _ptr(sel)
    if ret_state is not None and reward is not None:
        m = reward.numel()
        if n is not None and m != n:
            raise ValueError('reward must hold %d values, got %d' % (n, m))
        _dev(reward, 'reward', device=ret_state.device)
        reward_out = reward if reward_out is None else _dev(reward_out, 'reward_out', np.float32, tuple(reward.shape), ret_state.device)
        a.ret_scale, a.reward, a.reward_out, n = _ptr(ret_state.scale), _ptr(reward), _ptr(reward_out), m
        if done_code is not None:
            _dev(done_code, 'done_code', np.uint8, device=ret_state.device)
            _dev(ret_run, 'ret_run', np.float32, (m,), ret_state.device)
            a.done_code, a.ret_run = _ptr(done_code), _ptr(ret_run)
    a.n = 0 if n is None else n
    return a, out, reward_out


def apply(obs_state=None, x=None, out=None, clip=10., sel_x=None, sel=None, sel_value=0, ret_state=None, reward=None, reward_out=None,
          done_code=None, ret_run=None, clip_rew=10.):
    """eb_norm_apply: out [n, D] = clip((x - mean_f) / den_f) (out None: in place), the same in place on the rows of sel_x whose
    sel == sel_value, and reward_out = clip(reward / den_ret_f) with ret_run zeroed where done_code != 0.  ONE launch on the current stream;
    the states are only read.  -> (out, reward_out)"""
    a, out, reward_out = _apply_args(obs_state, x, out, clip, sel_x, sel, sel_value, ret_state, reward, reward_out, done_code, ret_run, clip_rew)
    api, dev = norm_api(), (obs_state if obs_state is not None else ret_state).device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.apply(C.byref(a)))
    return out, reward_out


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def _groups(D):
    return min(THREADS // D, ROWS)


def partial_sums_reference(x, K):
    """norm_partial_kernel and the fold over its blocks in NumPy: x [n, D] float32, K [D] float64 -> (S1 [D], S2 [D]) float64, the sums
    of (x - K) and (x - K)^2 in the kernels' order — lane (g, d) over the rows g, g + G, ... of its block's runs, the G lanes of a column by
    halving, the blocks ascending."""
    x = np.asarray(x, np.float32)
    n, D = x.shape
    K = np.asarray(K, np.float64).reshape(D)
    G = _groups(D)
    runs = -(-n // ROWS)
    blocks = min(runs, EB_NORM_MAX_BLOCKS)
    passes = -(-runs // blocks)
    padded = np.zeros((passes * blocks * ROWS, D), np.float64)
    padded[:n] = x
    valid = (np.arange(passes * blocks * ROWS) < n).reshape(passes, blocks, ROWS)
    v = (padded - K[None, :]).reshape(passes, blocks, ROWS, D)             # run k * blocks + b is block b's k-th
    a1, a2 = np.zeros((blocks, G, D)), np.zeros((blocks, G, D))
    with np.errstate(all='ignore'):
        for k in range(passes):
            for j in range(-(-ROWS // G)):
                rows = np.arange(G) + j * G                                 # lane group g reads row g + j G of the run
                inside = rows < ROWS
                r = np.where(inside, rows, 0)
                take = (valid[k][:, r] & inside[None, :])[:, :, None]
                d = v[k][:, r, :]
                a1 = np.where(take, a1 + d, a1)
                a2 = np.where(take, a2 + d * d, a2)
        P = 1
        while P < G:
            P *= 2
        w = P // 2
        while w:
            m = max(0, min(w, G - w))
            a1[:, :m] = a1[:, :m] + a1[:, w:w + m]
            a2[:, :m] = a2[:, :m] + a2[:, w:w + m]
            w //= 2
        S1, S2 = np.zeros(D), np.zeros(D)
        for b in range(blocks):
            S1 = S1 + a1[b, 0]
            S2 = S2 + a2[b, 0]
    return S1, S2


def _merge(state, S1, S2, K, n):
    """norm_fold_kernel's merge (update_mean_var_count_from_moments, preprocessor.py:14-25, in double) into `state`, in place"""
    D = state.D
    mean, var, count = state.stat[:D], state.stat[D:2 * D], state.stat[2 * D]
    N = np.float64(n)
    with np.errstate(all='ignore'):
        a = S1 / N
        bm = K + a
        bv = S2 / N - a * a
        bv = np.where(bv < 0.0, 0.0, bv)                                    # a NaN travels
        delta = bm - mean
        tot = count + N
        new_mean = mean + (delta * N) / tot
        M2 = (var * count + bv * N) + (((delta * delta) * count) * N) / tot
        new_var = M2 / tot
    state.stat = np.concatenate([new_mean, new_var, [tot]])
    state.scale = _scale_of(new_mean, new_var, state.eps_f)


def update_reference(state, x):
    """the observation part of eb_norm_update on a HostState, in place -> state.  x [n, D]; n = 0 changes nothing."""
    x = np.asarray(x, np.float32).reshape(-1, state.D)
    if x.shape[0]:
        K = state.scale[:state.D].astype(np.float64)                         # mean_f as it stood before
        S1, S2 = partial_sums_reference(x, K)
        _merge(state, S1, S2, K, x.shape[0])
    return state


def update_return_reference(state, reward, ret_run, gamma):
    """the return part of eb_norm_update: ret_run [n] (float32, in place) = ret_run * gamma + reward — one fp32 multiply, one fp32 add —
    and its n values merged into the width-1 HostState `state`, in place -> state"""
    reward = np.asarray(reward, np.float32).reshape(-1)
    if ret_run.dtype != np.float32 or ret_run.shape != reward.shape:
        raise ValueError('ret_run must be float32 %s' % (reward.shape,))
    with np.errstate(all='ignore'):
        ret_run[:] = (ret_run * np.float32(gamma)).astype(np.float32) + reward
    return update_reference(state, ret_run.reshape(-1, 1))


def _clip(v, c):
    c = np.float32(c)
    v = np.where(v < -c, -c, v)                                             # selects: a NaN travels
    return np.where(v > c, c, v).astype(np.float32)


def apply_reference(state, x, clip=10., sel=None, sel_value=0):
    """the observation parts of eb_norm_apply in NumPy: x [n, D] float32 -> clip((x - mean_f) / den_f), one fp32 subtraction and one fp32
    division; with `sel` [n] only the rows with sel == sel_value are normalised and the others returned as they are"""
    x = np.asarray(x, np.float32)
    D = state.D
    with np.errstate(all='ignore'):
        y = _clip(((x - state.scale[:D]).astype(np.float32) / state.scale[D:]).astype(np.float32), clip)
    if sel is not None:
        y = np.where((np.asarray(sel) == sel_value)[:, None], y, x)
    return y


def apply_reward_reference(state, reward, clip=10., done_code=None, ret_run=None):
    """the reward part of eb_norm_apply: -> clip(reward / den_ret_f), no mean subtraction; with done_code, ret_run [n] is zeroed in place
    where done_code != 0"""
    reward = np.asarray(reward, np.float32)
    with np.errstate(all='ignore'):
        out = _clip((reward / state.scale[1]).astype(np.float32), clip)
    if done_code is not None:
        ret_run[np.asarray(done_code).reshape(ret_run.shape) != 0] = np.float32(0)
    return out


# ---- the reference's Preprocessor over the device state --------------------------------------------------------------------------------------
class Preprocessor(object):
    """utils/preprocessor.py:59-182 with the statistics on the device.  `ob_shape`: D or (D,).  process_obs / process_rew /
    np_process_obses / np_process_rewards take a device tensor (or a DevArray) and return one; a NumPy array is uploaded and the result
    comes back as NumPy.  With num_agent = B the batched branches run ([B, D] observations, [B] rewards and dones); without it the
    single-env ones ([D], scalars).  process_rew resets the running return where done != 0 — the reference's single-env branch per env;
    its batched branch raises as written (include/envbuild_norm.h)."""

    def __init__(self, ob_shape, obs_ptype='normalize', rew_ptype='normalize', obs_scale=None, rew_scale=None, rew_shift=None, clipob=10.,
                 cliprew=10., gamma=0.99, epsilon=1e-8, device=None, **kwargs):
        from .dynamics_and_models import _resolve_device
        D = int(np.prod(ob_shape)) if np.ndim(ob_shape) else int(ob_shape)
        self.device = _resolve_device(device)
        self.obs_ptype, self.rew_ptype = obs_ptype, rew_ptype
        self.ob_rms = NormState(D, self.device, epsilon) if obs_ptype == 'normalize' else None
        self.ret_rms = NormState(1, self.device, epsilon) if rew_ptype == 'normalize' else None
        f32 = dict(dtype=torch.float32, device=self.device)
        self.obs_scale = torch.as_tensor(np.asarray(obs_scale, np.float32), **f32) if obs_ptype == 'scale' else None
        self.rew_scale = rew_scale if rew_ptype == 'scale' else None
        self.rew_shift = rew_shift if rew_ptype == 'scale' else None
        self.clipob, self.cliprew, self.gamma, self.epsilon = float(clipob), float(cliprew), float(gamma), float(epsilon)
        self.num_agent = kwargs.get('num_agent')
        self.ret = torch.zeros((self.num_agent or 1,), **f32)

    def _in(self, x, shape, dtype=torch.float32):
        host = not isinstance(_unwrap(x), torch.Tensor)
        t = _unwrap(x)
        t = torch.as_tensor(np.asarray(t), device=self.device) if host else t
        return t.to(device=self.device, dtype=dtype).reshape(shape).contiguous(), host

    @staticmethod
    def _out(t, host, shape=None):
        t = t if shape is None else t.reshape(shape)
        return t.cpu().numpy() if host else t

    def process_obs(self, obs):
        if self.obs_ptype == 'normalize':
            x, host = self._in(obs, (-1, self.ob_rms.D))
            y = torch.empty_like(x)
            update(self.ob_rms, x)
            apply(self.ob_rms, x, y, self.clipob)
            return self._out(y, host, None if self.num_agent is not None else (self.ob_rms.D,))
        return self.np_process_obses(obs)

    def process_rew(self, rew, done):
        if self.rew_ptype == 'normalize':
            r, host = self._in(rew, (-1,))
            d = _unwrap(done)
            d = (d != 0) if isinstance(d, torch.Tensor) else torch.as_tensor(np.asarray(d) != 0)
            d = d.to(device=self.device, dtype=torch.uint8).reshape(-1).contiguous()
            out = torch.empty_like(r)
            update(None, None, self.ret_rms, r, self.ret, self.gamma)
            apply(None, None, None, ret_state=self.ret_rms, reward=r, reward_out=out, done_code=d, ret_run=self.ret, clip_rew=self.cliprew)
            return self._out(out, host, None if self.num_agent is not None else ())
        return self.np_process_rewards(rew)

    def np_process_obses(self, obses):
        if self.obs_ptype == 'normalize':
            x, host = self._in(obses, (-1, self.ob_rms.D))
            y = torch.empty_like(x)
            apply(self.ob_rms, x, y, self.clipob)
            return self._out(y, host, np.shape(_unwrap(obses)))
        if self.obs_ptype == 'scale':
            x, host = self._in(obses, np.shape(_unwrap(obses)))
            return self._out(x * self.obs_scale, host)
        return obses

    def np_process_rewards(self, rewards):
        if self.rew_ptype == 'normalize':
            r, host = self._in(rewards, (-1,))
            out = torch.empty_like(r)
            apply(None, None, None, ret_state=self.ret_rms, reward=r, reward_out=out, clip_rew=self.cliprew)
            return self._out(out, host, np.shape(_unwrap(rewards)))
        if self.rew_ptype == 'scale':
            r, host = self._in(rewards, np.shape(_unwrap(rewards)))
            return self._out((r + self.rew_shift) * self.rew_scale, host)
        return rewards

    def get_params(self):
        tmp = {}
        if self.ob_rms:
            tmp['ob_rms'] = self.ob_rms.get_params()
        if self.ret_rms:
            mean, var, count = self.ret_rms.get_params()
            tmp['ret_rms'] = (mean.reshape(()), var.reshape(()), count)            # shape (), as the reference's
        return tmp

    def set_params(self, params):
        if self.ob_rms and 'ob_rms' in params:
            self.ob_rms.set_params(*params['ob_rms'])
        if self.ret_rms and 'ret_rms' in params:
            self.ret_rms.set_params(*params['ret_rms'])

    def save_params(self, save_dir, npy=False):
        """save_dir/ppc_params.npz (arrays only); npy=True writes the reference's ppc_params.npy, a pickled dict"""
        params = self.get_params()
        if npy:
            np.save(os.path.join(save_dir, 'ppc_params.npy'), params)
            return
        arrays = {}
        for k, (mean, var, count) in params.items():
            arrays.update({k + '_mean': mean, k + '_var': var, k + '_count': np.float64(count)})
        np.savez(os.path.join(save_dir, 'ppc_params.npz'), **arrays)

    def load_params(self, load_dir):
        """from load_dir/ppc_params.npz, else the reference's load_dir/ppc_params.npy"""
        for name in ('ppc_params.npz', 'ppc_params.npy'):
            path = os.path.join(load_dir, name)
            if os.path.isfile(path):
                self.set_params(_read_params(path))
                return
        raise FileNotFoundError('no ppc_params.npz or ppc_params.npy in %s' % load_dir)


# ---- the collector ----------------------------------------------------------------------------------------------------------------------------
class Collector(_collect.Collector):
    """collect.Collector with the observations and rewards normalised on their way into the rollout buffer.  The same buffers, finish(),
    episodes() and returned dict; only collect() differs:

        collect():   eb_collect_begin(env's observation -> obs_buf[0])
                     obs_buf[0]: iteration 0: eb_norm_update + eb_norm_apply in place; later iterations: eb_norm_apply alone — that
                         observation was counted at the last step of the iteration before and the state has not moved since, so
                         obs_buf[0] repeats that iteration's obs_buf[T] bit for bit
                     for t in 0 .. T - 1:
                         eb_policy_sample(obs_buf[t]); env.step; eb_collect_record(t) on the RAW step outputs
                         eb_norm_update(observation part: obs_buf[t + 1]; return part: rew_buf[t])                       (2 kernels)
                         eb_norm_apply(obs_buf[t + 1] in place; the rows of trunc_obs with trunc_t == t; rew_buf[t] in place, ret_run
                             zeroed where code_buf[t] != 0)                                                                (1 kernel)

    ret_buf and the episode log therefore stay RAW returns; the final observations of truncated episodes are normalised, not counted.
    `obs_state` (width D), `ret_state` (width 1) and `ret_run` [B] live on the device.  update=False freezes the statistics (evaluation):
    only eb_norm_apply is launched and ret_run is left alone.  norm_obs / norm_reward switch the two halves.  The networks see normalised
    observations: they carry no obs_scale of their own."""

    def __init__(self, env, policy, value, steps, action_range, seed=0, gamma=0.99, clipob=10., cliprew=10., norm_obs=True, norm_reward=True,
                 update=True, epsilon=1e-8):
        super(Collector, self).__init__(env, policy, value, steps, action_range, seed=seed)
        if not (norm_obs or norm_reward):
            raise ValueError('norm.Collector normalises observations, rewards or both; collect.Collector does neither')
        for name, v in (('gamma', gamma), ('clipob', clipob), ('cliprew', cliprew)):
            if not np.isfinite(v):
                raise ValueError('%s must be finite, got %r' % (name, v))
        T, B, D, dev = self.steps, self.n_env, self.obs_dim, self.device
        self.norm_obs, self.norm_reward, self.update_stats = bool(norm_obs), bool(norm_reward), bool(update)
        self.gamma, self.clipob, self.cliprew = float(gamma), float(clipob), float(cliprew)
        self.obs_state, self.ret_state = NormState(D, dev, epsilon), NormState(1, dev, epsilon)
        self.ret_run = torch.zeros((B,), dtype=torch.float32, device=dev)
        self.norm = norm_api()
        buf = self.buf
        obs_state = self.obs_state if self.norm_obs else None
        ret_state = self.ret_state if self.norm_reward else None
        self._first_update = _update_args(self.obs_state, buf['obs_buf'][0]) if self.norm_obs else None
        self._first_apply = _apply_args(self.obs_state, buf['obs_buf'][0], None, self.clipob)[0] if self.norm_obs else None
        self._updates = [_update_args(obs_state, buf['obs_buf'][t + 1] if self.norm_obs else None, ret_state,
                                      buf['rew_buf'][t] if self.norm_reward else None, self.ret_run, self.gamma) for t in range(T)]
        self._applies, self._frozen = [], []
        for t in range(T):
            obs = dict(x=buf['obs_buf'][t + 1], sel_x=buf['trunc_obs'], sel=buf['trunc_t'], sel_value=t) if self.norm_obs else {}
            rew = dict(ret_state=ret_state, reward=buf['rew_buf'][t], clip_rew=self.cliprew) if self.norm_reward else {}
            self._applies.append(_apply_args(obs_state, clip=self.clipob, done_code=buf['code_buf'][t] if self.norm_reward else None,
                                             ret_run=self.ret_run if self.norm_reward else None, **dict(obs, **rew))[0])
            self._frozen.append(_apply_args(obs_state, clip=self.clipob, **dict(obs, **rew))[0])

    def collect(self):
        """T steps from the env's current observation into the buffer, normalised; the env is left T steps further"""
        api, norm, env, pol, T, B = self.api, self.norm, self.env, self.policy, self.steps, self.n_env
        moving = self.update_stats
        applies = self._applies if moving else self._frozen
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            h = pol._handle
            a = self._begin
            a.obs, a.stream = env.obs.t.data_ptr(), s
            api.check(api.begin(C.byref(a)))
            if self.norm_obs:
                if moving and self.iteration == 0:
                    self._first_update.stream = s
                    norm.check(norm.update(C.byref(self._first_update)))
                self._first_apply.stream = s
                norm.check(norm.apply(C.byref(self._first_apply)))
            base = self.iteration * T
            for t in range(T):
                pol.api.check(self._sample(h, B, self._obs_at[t], None, None, self.seed, base + t, self.action_range,
                                           self._act_at[t].data_ptr(), None, self._logit_at[t], None, s))
                obs, reward, _done, info = env.step(self._act_at[t])
                r = self._records[t]
                _collect._set_step(r, obs.t, reward.t, env.done_code, info['final_observation'].t)
                r.stream = s
                api.check(api.record(C.byref(r)))
                if moving:
                    u = self._updates[t]
                    u.stream = s
                    norm.check(norm.update(C.byref(u)))
                n = applies[t]
                n.stream = s
                norm.check(norm.apply(C.byref(n)))
        self.iteration += 1
