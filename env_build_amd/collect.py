"""The collection phase of a PPO iteration as library launches (include/envbuild_collect.h, env_build_amd/csrc/eb_collect.hip): the rollout
buffer one env step is recorded into with ONE launch — observation slot, reward, eb_gae's truncation flags, the final observation of a
time-limit truncation, the running episode return and length — the bootstrap values of the truncated steps (ONE launch), the episode
statistics (ONE launch of 64 blocks, folded on the host when read), and `Collector`, which strings them around `eb_policy_sample`,
`CrossroadEnd2end.step`, `eb_mlp_forward`, `eb_policy_logp_from_logits` and `eb_gae` and hands `epoch.PPOEpochs` its data.

`begin(obs, obs_buf, trunc_t)`: eb_collect_begin.  `record(t, obs, reward, done_code, final_obs, buf)`: eb_collect_record into the dict
of buffers `buffers(T, B, D)` makes.  `next_values(values, v_trunc, trunc_t, out)`: eb_collect_next_values.
`episode_log(ret_buf, len_buf, code_buf, out)`: eb_collect_episode_log into out [64, 16] float64; `fold_episode_log(out)` folds a host copy.
`begin_reference`, `record_reference`, `next_values_reference` and `episode_log_reference` restate the header's contract in NumPy, in
the kernels' own order.

The entries live in env_build_amd/lib/libenvbuild_collect.so, a library of its own that is bound here on first use (COLLECT_PROTOTYPES):
the other three libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from .dynamics_and_models import _stream

__all__ = ['begin', 'record', 'next_values', 'episode_log', 'fold_episode_log', 'buffers', 'Collector', 'begin_reference', 'record_reference',
           'next_values_reference', 'episode_log_reference', 'EbCollectBeginArgs', 'EbCollectRecordArgs', 'EbCollectNextValuesArgs',
           'EbCollectEpisodeLogArgs', 'EB_COLLECT_ABI_VERSION', 'EB_COLLECT_LOG_BLOCKS', 'EB_COLLECT_LOG_FIELDS', 'COLLECT_PROTOTYPES',
           'collect_api']

_P, _I, _L = C.c_void_p, C.c_int32, C.c_int64
EB_COLLECT_ABI_VERSION = 1
EB_COLLECT_LOG_BLOCKS = 64
EB_COLLECT_LOG_FIELDS = 16
THREADS = 256                                                  # of every kernel (csrc/eb_collect_device.h)
TIME_LIMIT = _capi.DONE_NAMES.index('time_limit')              # EB_DONE_TIME_LIMIT
HEADER = 'envbuild_collect.h'
BUFFERS = (('obs_buf', np.float32), ('rew_buf', np.float32), ('nonterminal', np.float32), ('carry', np.float32), ('ret_buf', np.float32),
           ('len_buf', np.int32), ('code_buf', np.uint8), ('trunc_obs', np.float32), ('trunc_t', np.int32), ('ep_ret', np.float32),
           ('ep_len', np.int32))


class EbCollectBeginArgs(C.Structure):
    """eb_collect_begin_args of include/envbuild_collect.h"""
    _fields_ = [('n_env', _I), ('obs_dim', _I), ('obs', _P), ('obs_buf', _P), ('trunc_t', _P), ('stream', _P)]


class EbCollectRecordArgs(C.Structure):
    """eb_collect_record_args"""
    _fields_ = [('n_env', _I), ('obs_dim', _I), ('steps', _I), ('t', _I), ('obs', _P), ('reward', _P), ('done_code', _P), ('final_obs', _P),
                ('ep_ret', _P), ('ep_len', _P), ('obs_buf', _P), ('rew_buf', _P), ('nonterminal', _P), ('carry', _P), ('ret_buf', _P),
                ('len_buf', _P), ('code_buf', _P), ('trunc_obs', _P), ('trunc_t', _P), ('stream', _P)]


class EbCollectNextValuesArgs(C.Structure):
    """eb_collect_next_values_args"""
    _fields_ = [('n_env', _I), ('steps', _I), ('values', _P), ('v_trunc', _P), ('trunc_t', _P), ('next_values', _P), ('stream', _P)]


class EbCollectEpisodeLogArgs(C.Structure):
    """eb_collect_episode_log_args"""
    _fields_ = [('n_slots', _L), ('ret_buf', _P), ('len_buf', _P), ('code_buf', _P), ('out', _P), ('stream', _P)]


# include/envbuild_collect.h: name -> (restype, argtypes) for every symbol the header declares
COLLECT_PROTOTYPES = {
    'eb_collect_abi_version': (C.c_int, []),
    'eb_collect_last_error': (C.c_char_p, []),
    'eb_collect_begin': (C.c_int, [C.POINTER(EbCollectBeginArgs)]),
    'eb_collect_record': (C.c_int, [C.POINTER(EbCollectRecordArgs)]),
    'eb_collect_next_values': (C.c_int, [C.POINTER(EbCollectNextValuesArgs)]),
    'eb_collect_episode_log': (C.c_int, [C.POINTER(EbCollectEpisodeLogArgs)]),
}


class CollectApi(object):
    """libenvbuild_collect.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in COLLECT_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in COLLECT_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_collect_abi_version()
        if v != EB_COLLECT_ABI_VERSION:
            raise _capi.EbError('%s: collect ABI version %d, expected %d (include/%s)' % (path, v, EB_COLLECT_ABI_VERSION, HEADER))
        self.begin, self.record = self.lib.eb_collect_begin, self.lib.eb_collect_record
        self.next_values, self.episode_log = self.lib.eb_collect_next_values, self.lib.eb_collect_episode_log

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_collect_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(collect): %s' % msg)
            raise _capi.EbError('envbuild(collect) error %d: %s' % (rc, msg))


_collect_api = None


def collect_api():
    """The collection library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls
    back — when it is absent or was built from other sources and cannot be rebuilt."""
    global _collect_api
    if _collect_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.collect_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.COLLECT_LIB, _build.CSRC))
            try:
                _build.build_collect()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.COLLECT_LIB, e))
        _collect_api = CollectApi(_build.COLLECT_LIB)
    return _collect_api


def _ptr(t):
    return None if t is None else t.data_ptr()


_TORCH = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8, np.float64: torch.float64}


def _dev(t, what, dtype=np.float32, shape=None, device=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == _TORCH[dtype] and t.is_contiguous()):
        raise TypeError('%s must be a contiguous %s device tensor (there is no CPU path)' % (what, np.dtype(dtype).name))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s, got %s' % (what, tuple(shape), tuple(t.shape)))
    if device is not None and t.device != device:
        raise ValueError('%s must live on %s' % (what, device))
    return t


def _shapes(T, B, D):
    return dict(obs_buf=(T + 1, B, D), rew_buf=(T, B), nonterminal=(T, B), carry=(T, B), ret_buf=(T, B), len_buf=(T, B), code_buf=(T, B),
                trunc_obs=(B, D), trunc_t=(B,), ep_ret=(B,), ep_len=(B,))


def buffers(T, B, D, device=None):
    """the rollout buffer of T steps x B envs x D floats: a dict of device tensors named as the header names them, every array zero and
    trunc_t -1; NumPy arrays with device None (what the restatements work on)"""
    shapes = _shapes(int(T), int(B), int(D))
    if device is None:
        out = {k: np.zeros(shapes[k], dt) for k, dt in BUFFERS}
    else:
        out = {k: torch.zeros(shapes[k], dtype=_TORCH[dt], device=device) for k, dt in BUFFERS}
    out['trunc_t'][...] = -1
    return out


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def _begin_args(obs, obs_buf, trunc_t):
    B, D = obs.shape
    _dev(obs, 'obs')
    _dev(obs_buf, 'obs_buf', device=obs.device)
    if obs_buf.dim() != 3 or tuple(obs_buf.shape[1:]) != (B, D) or obs_buf.shape[0] < 2:
        raise ValueError('obs_buf must be [T + 1, %d, %d], got %s' % (B, D, tuple(obs_buf.shape)))
    _dev(trunc_t, 'trunc_t', np.int32, (B,), obs.device)
    return EbCollectBeginArgs(n_env=B, obs_dim=D, obs=_ptr(obs), obs_buf=_ptr(obs_buf), trunc_t=_ptr(trunc_t))


def begin(obs, obs_buf, trunc_t):
    """eb_collect_begin: obs_buf[0] = obs [B, D] and trunc_t [B] = -1.  ONE launch on the current stream."""
    a = _begin_args(obs, obs_buf, trunc_t)
    api, dev = collect_api(), obs.device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.begin(C.byref(a)))


def _record_args(t, buf, obs=None, reward=None, done_code=None, final_obs=None):
    """eb_collect_record_args for step t into `buf`; the step's four inputs may be set later (`_set_step`)"""
    T, B, D = buf['obs_buf'].shape[0] - 1, buf['obs_buf'].shape[1], buf['obs_buf'].shape[2]
    dev = buf['obs_buf'].device
    shapes = _shapes(T, B, D)
    for k, dt in BUFFERS:
        _dev(buf[k], k, dt, shapes[k], dev)
    a = EbCollectRecordArgs(n_env=B, obs_dim=D, steps=T, t=int(t), **{k: _ptr(buf[k]) for k, _ in BUFFERS})
    if obs is not None:
        _set_step(a, _dev(obs, 'obs', np.float32, (B, D), dev), _dev(reward, 'reward', np.float32, (B,), dev),
                  _dev(done_code, 'done_code', np.uint8, (B,), dev),
                  None if final_obs is None else _dev(final_obs, 'final_obs', np.float32, (B, D), dev))
    return a


def _set_step(a, obs, reward, done_code, final_obs):
    a.obs, a.reward, a.done_code, a.final_obs = obs.data_ptr(), reward.data_ptr(), done_code.data_ptr(), _ptr(final_obs)


def record(t, obs, reward, done_code, final_obs, buf):
    """eb_collect_record: step t of `buf` (a dict as `buffers` makes) from obs [B, D] (after the step), reward [B], done_code [B] uint8 and
    final_obs [B, D] or None (a time-limit code is then a termination).  ONE launch on the current stream."""
    a = _record_args(t, buf, obs, reward, done_code, final_obs)
    api, dev = collect_api(), obs.device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.record(C.byref(a)))


def _next_values_args(values, v_trunc, trunc_t, out):
    _dev(values, 'values')
    if values.dim() != 2 or values.shape[0] < 1:
        raise ValueError('values must be [T + 1, B], got %s' % (tuple(values.shape),))
    T, B = values.shape[0] - 1, values.shape[1]
    _dev(v_trunc, 'v_trunc', np.float32, (B,), values.device)
    _dev(trunc_t, 'trunc_t', np.int32, (B,), values.device)
    _dev(out, 'next_values', np.float32, (T, B), values.device)
    return EbCollectNextValuesArgs(n_env=B, steps=T, values=_ptr(values), v_trunc=_ptr(v_trunc), trunc_t=_ptr(trunc_t), next_values=_ptr(out))


def next_values(values, v_trunc, trunc_t, out):
    """eb_collect_next_values: out [T, B] = v_trunc [B] where trunc_t [B] names the step, else values [T + 1, B]'s next row.  ONE launch."""
    a = _next_values_args(values, v_trunc, trunc_t, out)
    api, dev = collect_api(), values.device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.next_values(C.byref(a)))
    return out


def _episode_log_args(ret_buf, len_buf, code_buf, out):
    n = int(ret_buf.numel())
    _dev(ret_buf, 'ret_buf')
    for t, what, dt in ((len_buf, 'len_buf', np.int32), (code_buf, 'code_buf', np.uint8)):
        if _dev(t, what, dt, device=ret_buf.device).numel() != n:
            raise ValueError('%s must hold %d slots, got %d' % (what, n, t.numel()))
    if _dev(out, 'out', np.float64, device=ret_buf.device).numel() != EB_COLLECT_LOG_BLOCKS * EB_COLLECT_LOG_FIELDS:
        raise ValueError('out must be %d x %d' % (EB_COLLECT_LOG_BLOCKS, EB_COLLECT_LOG_FIELDS))
    return EbCollectEpisodeLogArgs(n_slots=n, ret_buf=_ptr(ret_buf), len_buf=_ptr(len_buf), code_buf=_ptr(code_buf), out=_ptr(out))


def episode_log(ret_buf, len_buf, code_buf, out):
    """eb_collect_episode_log: the slots of ret_buf, len_buf (int32) and code_buf (uint8) -> out [64, 16] float64 on the device, the
    per-block figures `fold_episode_log` reads.  ONE launch, no host read."""
    a = _episode_log_args(ret_buf, len_buf, code_buf, out)
    api, dev = collect_api(), out.device
    with torch.cuda.device(dev):
        a.stream = _stream(dev)
        api.check(api.episode_log(C.byref(a)))
    return out


def fold_episode_log(out):
    """out [64, 16] (a HOST copy of eb_collect_episode_log's blocks) -> dict: episodes (the finished slots), return_mean, return_std (of
    the population), length_mean, return_max, return_min, nonfinite (finished slots whose return is a NaN or an infinity), outcomes
    {name of _capi.DONE_NAMES: slots with that code} and slots.  The blocks are added in ascending order.  Without a finished slot the
    five return and length figures are NaN.  With nonfinite > 0 they are not to be trusted: a NaN return is left out of the sums and
    of the maximum and minimum, but not of the count they are divided by."""
    out = np.asarray(out, np.float64)
    if out.shape != (EB_COLLECT_LOG_BLOCKS, EB_COLLECT_LOG_FIELDS):
        raise ValueError('fold_episode_log takes [%d, %d], got %s' % (EB_COLLECT_LOG_BLOCKS, EB_COLLECT_LOG_FIELDS, out.shape))
    nan = float('nan')
    with np.errstate(all='ignore'):                          # (the maximum and minimum columns are not sums: their totals are not used)
        total = out[0].copy()
        for b in range(1, EB_COLLECT_LOG_BLOCKS):
            total = total + out[b]
        n = total[0]
        mean = total[1] / n if n else nan
        var = total[2] / n - mean * mean if n else nan
        return dict(episodes=int(n), return_mean=float(mean), return_std=float(np.sqrt(var if var > 0.0 or var != var else 0.0)),
                    length_mean=float(total[3] / n) if n else nan, return_max=float(out[:, 4].max()) if n else nan,
                    return_min=float(out[:, 5].min()) if n else nan, nonfinite=int(total[6]),
                    outcomes={name: int(total[7 + k]) for k, name in enumerate(_capi.DONE_NAMES)}, slots=int(total[15]))


# ---- the collector --------------------------------------------------------------------------------------------------------------------------
class Collector(object):
    """T = `steps` env steps of B envs into a rollout buffer, and the head of the update — values, bootstrap values of the truncated
    steps, logp_old, advantages and returns — on the current stream, everything a library launch:

        collect():   eb_collect_begin(env's observation -> obs_buf[0])                                          (1 kernel)
                     for t in 0 .. T - 1:
                         eb_policy_sample(obs_buf[t] -> act_buf[t], logit_buf[t]; counter = iteration * T + t)   (1 kernel)
                         env.step(act_buf[t])                                                                   (eb_env_step)
                         eb_collect_record(t)                                                                   (1 kernel)
        finish(gamma, lam):
                     eb_mlp_forward(value, obs_buf [(T + 1) * B, D] -> values [T + 1, B])
                     eb_mlp_forward(value, trunc_obs [B, D] -> v_trunc [B])
                     eb_collect_next_values
                     eb_policy_logp_from_logits(logit_buf, act_buf -> logp_old)
                     eb_gae(rew_buf, values, nonterminal, next_values, carry -> adv, ret)
                     -> dict(obs, actions, logp_old, adv, ret, v_old): what epoch.PPOEpochs takes
        episodes():  eb_collect_episode_log, one device-to-host copy, fold_episode_log

    `env`: a CrossroadEnd2end with auto_reset=True, copy_outputs=False and n_env > 1.  `policy`: an fp32 MLPNet / TrainableMLPNet with
    2 * act_dim outputs (eb_policy_sample_supported); `value`: one with 1 output.  steps <= env.max_episode_steps, so that an env
    truncates at most once per collection and one trunc_obs row per env suffices (include/envbuild_collect.h).  A time-limit truncation
    bootstraps from the value of its final observation; every other ending is a termination.  The logits recorded while sampling give
    logp_old from one elementwise launch, the bits eb_policy_logp would give on the same rows.  Every buffer is allocated and every
    argument struct prepared here, once; the tensors finish() returns are views of them, refilled in place at every iteration, so one
    captured PPOEpochs graph keeps replaying.  collect() and finish() make no torch operation of their own, no allocation and no host
    read.  The collection is issued eagerly: CrossroadEnd2end.step passes its respawn and reset counters by value."""

    def __init__(self, env, policy, value, steps, action_range, seed=0):
        from . import policy_logp, policy_sample, ppo
        from .endtoend import CrossroadEnd2end
        from .policy import MLPNet
        if not isinstance(env, CrossroadEnd2end):
            raise TypeError('Collector drives a CrossroadEnd2end, got %s' % type(env).__name__)
        if not env.auto_reset or env.copy_outputs or env.n_env < 2:
            raise ValueError('Collector needs an env with auto_reset=True, copy_outputs=False and n_env > 1')
        if not isinstance(policy, MLPNet) or not isinstance(value, MLPNet):
            raise TypeError('policy and value must be MLPNets')
        T, B, D = int(steps), env.n_env, env.obs_dim
        if T < 1 or T > 65535:
            raise ValueError('steps must be in 1 .. 65535 (eb_gae), got %d' % T)
        if env.max_episode_steps is not None and T > env.max_episode_steps:
            raise ValueError('steps = %d exceeds env.max_episode_steps = %d: an env could be truncated twice within one collection, and the '
                             'buffer keeps one final observation per env' % (T, env.max_episode_steps))
        dev = env.device
        if policy.device != dev or value.device != dev:
            raise ValueError('the networks must live on the device of the env')
        if policy.input_dim != D or value.input_dim != D or value.output_dim != 1 or policy.output_dim < 2 or policy.output_dim % 2:
            raise ValueError('the policy must map %d -> 2 * act_dim and the value network %d -> 1' % (D, D))
        A = policy.output_dim // 2
        if A != env.action_number:
            raise ValueError('the policy has %d actions, the env takes %d' % (A, env.action_number))
        if not policy_sample._supported(policy):
            raise ValueError('Collector: eb_policy_sample_supported refuses the policy %s (precision %r): an fp16 handle has no fused sampling '
                             'launch, and fp16 policies are not collected with' % (policy.name, policy.precision))
        if value.precision != 'fp32':
            raise ValueError('Collector: the value network %s must be fp32, got %r' % (value.name, value.precision))
        self.env, self.policy, self.value = env, policy, value
        self.steps, self.n_env, self.obs_dim, self.act_dim, self.device = T, B, D, A, dev
        self.action_range, self.seed, self.iteration = policy_sample._range(action_range), int(seed) & ((1 << 64) - 1), 0
        f32 = dict(dtype=torch.float32, device=dev)
        self.buf = buffers(T, B, D, dev)
        self.act_buf, self.logit_buf = torch.zeros((T, B, A), **f32), torch.zeros((T, B, 2 * A), **f32)
        self.values, self.v_trunc = torch.zeros((T + 1, B), **f32), torch.zeros((B,), **f32)
        self.next_values, self.logp_old = torch.zeros((T, B), **f32), torch.zeros((T * B,), **f32)
        self.adv, self.ret = torch.zeros((T, B), **f32), torch.zeros((T, B), **f32)
        self.log_blocks = torch.zeros((EB_COLLECT_LOG_BLOCKS, EB_COLLECT_LOG_FIELDS), dtype=torch.float64, device=dev)
        self.api = collect_api()
        self._sample = policy_sample.bind(policy.api)['eb_policy_sample']
        self._logp_fn = policy_logp.bind(policy.api)['eb_policy_logp_from_logits']
        self._gae_fn = ppo.bind(policy.api)['eb_gae']
        obs_buf = self.buf['obs_buf']
        self._obs_at = [obs_buf[t].data_ptr() for t in range(T)]
        self._act_at = [self.act_buf[t] for t in range(T)]                  # what env.step takes: views made once
        self._logit_at = [self.logit_buf[t].data_ptr() for t in range(T)]
        self._begin = EbCollectBeginArgs(n_env=B, obs_dim=D, obs_buf=_ptr(obs_buf), trunc_t=_ptr(self.buf['trunc_t']))
        self._records = [_record_args(t, self.buf) for t in range(T)]
        self._next = _next_values_args(self.values, self.v_trunc, self.buf['trunc_t'], self.next_values)
        self._logp = policy_logp._args(None, T * B, 2 * A, self.action_range, logits=self.logit_buf, actions=self.act_buf, logp=self.logp_old)
        self._gae = ppo._gae_args(None, T, B, 0.0, 0.0, rewards=self.buf['rew_buf'], values=self.values, nonterminal=self.buf['nonterminal'],
                                  next_values=self.next_values, carry=self.buf['carry'], adv=self.adv, ret=self.ret)
        self._log = _episode_log_args(self.buf['ret_buf'], self.buf['len_buf'], self.buf['code_buf'], self.log_blocks)
        self.data = dict(obs=obs_buf[:T].view(T * B, D), actions=self.act_buf.view(T * B, A), logp_old=self.logp_old, adv=self.adv.view(T * B),
                         ret=self.ret.view(T * B), v_old=self.values[:T].view(T * B))

    def collect(self):
        """T steps from the env's current observation into the buffer; the env is left T steps further"""
        api, env, pol, T, B = self.api, self.env, self.policy, self.steps, self.n_env
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            h = pol._handle                                       # (a TrainableMLPNet uploads weights written since the last launch)
            a = self._begin
            a.obs, a.stream = env.obs.t.data_ptr(), s
            api.check(api.begin(C.byref(a)))
            base = self.iteration * T
            for t in range(T):
                pol.api.check(self._sample(h, B, self._obs_at[t], None, None, self.seed, base + t, self.action_range,
                                           self._act_at[t].data_ptr(), None, self._logit_at[t], None, s))
                obs, reward, _done, info = env.step(self._act_at[t])
                r = self._records[t]
                _set_step(r, obs.t, reward.t, env.done_code, info['final_observation'].t)
                r.stream = s
                api.check(api.record(C.byref(r)))
        self.iteration += 1

    def finish(self, gamma, lam):
        """the head of the update on what collect() left -> the dict epoch.PPOEpochs takes (views of this object's buffers)"""
        api, val, T, B = self.api, self.value, self.steps, self.n_env
        g, l = float(gamma), float(lam)
        if not (np.isfinite(g) and np.isfinite(l)):
            raise ValueError('gamma and lam must be finite, got %r and %r' % (gamma, lam))
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            h = val._handle
            val.api.mlp_forward(h, (T + 1) * B, C.c_void_p(self.buf['obs_buf'].data_ptr()), C.c_void_p(self.values.data_ptr()), s)
            val.api.mlp_forward(h, B, C.c_void_p(self.buf['trunc_obs'].data_ptr()), C.c_void_p(self.v_trunc.data_ptr()), s)
            self._next.stream = s
            api.check(api.next_values(C.byref(self._next)))
            self._logp.stream = s
            self.policy.api.check(self._logp_fn(C.byref(self._logp)))
            self._gae.gamma, self._gae.lam, self._gae.stream = g, l, s
            self.policy.api.check(self._gae_fn(C.byref(self._gae)))
        return self.data

    def episodes(self):
        """the statistics of the episodes that ended within the last collection: one launch, one device-to-host copy, fold_episode_log"""
        with torch.cuda.device(self.device):
            self._log.stream = _stream(self.device)
            self.api.check(self.api.episode_log(C.byref(self._log)))
        return fold_episode_log(self.log_blocks.cpu().numpy())


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def begin_reference(buf, obs):
    """eb_collect_begin on a dict of NumPy arrays (`buffers(T, B, D)`), in place -> buf"""
    buf['obs_buf'][0] = np.asarray(obs, np.float32)
    buf['trunc_t'][:] = -1
    return buf


def record_reference(buf, t, obs, reward, done_code, final_obs=None):
    """eb_collect_record on a dict of NumPy arrays (`buffers(T, B, D)`), in place -> buf: step t from obs [B, D], reward [B], done_code
    [B] and final_obs [B, D] or None.  Every operation is the kernel's: one fp32 addition for the return."""
    obs, reward, c = np.asarray(obs, np.float32), np.asarray(reward, np.float32), np.asarray(done_code, np.uint8)
    T = buf['rew_buf'].shape[0]
    if not 0 <= t < T:
        raise ValueError('t must be in [0, %d)' % T)
    live = c == 0
    trunc = (c == TIME_LIMIT) & (final_obs is not None)
    buf['obs_buf'][t + 1] = obs
    buf['rew_buf'][t] = reward
    buf['nonterminal'][t] = np.where(live | trunc, np.float32(1), np.float32(0))
    buf['carry'][t] = np.where(live, np.float32(1), np.float32(0))
    if final_obs is not None:
        buf['trunc_obs'][trunc] = np.asarray(final_obs, np.float32)[trunc]
        buf['trunc_t'][trunc] = t
    with np.errstate(all='ignore'):
        R = (buf['ep_ret'] + reward).astype(np.float32)
    L = buf['ep_len'] + np.int32(1)
    buf['ret_buf'][t], buf['len_buf'][t], buf['code_buf'][t] = R, L, c
    buf['ep_ret'][:] = np.where(c != 0, np.float32(0), R)
    buf['ep_len'][:] = np.where(c != 0, np.int32(0), L)
    return buf


def next_values_reference(values, v_trunc, trunc_t):
    """eb_collect_next_values in NumPy: values [T + 1, B], v_trunc [B], trunc_t [B] -> [T, B].  A select: nothing is computed with an
    unused v_trunc row."""
    values, v_trunc, trunc_t = np.asarray(values, np.float32), np.asarray(v_trunc, np.float32), np.asarray(trunc_t)
    T = values.shape[0] - 1
    return np.where(trunc_t[None, :] == np.arange(T)[:, None], v_trunc[None, :], values[1:]).astype(np.float32)


def _halve(a, op=np.add):
    """x[t] = op(x[t], x[t + w]) for w = 128 .. 1 along the last axis of 256 -> the last axis' element 0"""
    a = a.copy()
    w = THREADS // 2
    while w:
        a[..., :w] = op(a[..., :w], a[..., w:2 * w])
        w //= 2
    return a[..., 0]


def episode_log_reference(ret_buf, len_buf, code_buf):
    """eb_collect_episode_log in NumPy on the slots of ret_buf (float32), len_buf (int32) and code_buf (uint8), flattened -> [64, 16]
    float64, the kernel's blocks in the kernel's order"""
    R = np.asarray(ret_buf, np.float32).reshape(-1)
    Ln = np.asarray(len_buf, np.int32).reshape(-1)
    c = np.asarray(code_buf, np.uint8).reshape(-1)
    n = R.size
    if Ln.size != n or c.size != n:
        raise ValueError('ret_buf, len_buf and code_buf must hold the same slots')
    span = EB_COLLECT_LOG_BLOCKS * THREADS
    rounds = max(1, -(-n // span))

    def cells(a, fill=0.0):
        out = np.full(rounds * span, fill, np.float64)
        out[:n] = a
        return out.reshape(rounds, EB_COLLECT_LOG_BLOCKS, THREADS)

    def total(x):                                                        # lane by lane in ascending slots, then the halving
        acc = np.zeros((EB_COLLECT_LOG_BLOCKS, THREADS))
        for r in range(rounds):
            acc = acc + x[r]
        return _halve(acc)

    out = np.zeros((EB_COLLECT_LOG_BLOCKS, EB_COLLECT_LOG_FIELDS))
    with np.errstate(all='ignore'):
        done = c != 0
        counted = done & ~np.isnan(R)
        R64 = R.astype(np.float64)
        out[:, 0] = total(cells(done.astype(np.float64)))
        out[:, 1] = total(cells(np.where(counted, R64, 0.0)))
        out[:, 2] = total(cells(np.where(counted, R64 * R64, 0.0)))
        out[:, 3] = total(cells(np.where(done, Ln.astype(np.float64), 0.0)))
        out[:, 4] = cells(np.where(counted, R64, -np.inf), -np.inf).max(axis=(0, 2))
        out[:, 5] = cells(np.where(counted, R64, np.inf), np.inf).min(axis=(0, 2))
        out[:, 6] = total(cells((done & ~np.isfinite(R)).astype(np.float64)))
        for k in range(8):
            out[:, 7 + k] = total(cells((c == k).astype(np.float64)))
        out[:, 15] = total(cells(np.ones(n)))
    return out
