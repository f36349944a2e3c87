"""Off-policy training on the device (include/envbuild_offpolicy.h, env_build_amd/csrc/eb_offpolicy.hip): a replay ring and the
memory-bound and elementwise work of a SAC update between the network launches the other libraries already have, as library launches —
`push`, `sample`, `q_pack`, `sac_critic`, `sac_actor`, `q_action_grad`, `polyak` — and the Python that strings them together:

`ReplayBuffer(capacity, obs_dim, act_dim, device)`: the ring and its fill word on the device, the cursor on the host.
`Collector(env, policy, buffer, action_range, seed)`: eb_policy_sample, env.step and ONE eb_replay_push per env step.
`SAC(policy, q1, q2, buffer, batch, ...)`: one SAC update as a fixed, capturable chain of launches; `capture()`, `replay()`, `log()`.
`push_reference`, `sample_index_reference`, `sample_reference`, `q_pack_reference`, `critic_reference`, `actor_reference`,
`action_grad_reference` and `polyak_reference` restate the header's contract in NumPy, in the kernels' own order: the GPU is held to them
bit for bit.

The entries live in env_build_amd/lib/libenvbuild_offpolicy.so, a library of its own that is bound here on first use
(OFFPOLICY_PROTOTYPES): the other seven libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no
CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from . import collect as _collect
from .dynamics_and_models import _stream
from .policy_sample import _GOLDEN, _exp_det, _fmaf, _splitmix64

__all__ = ['ReplayBuffer', 'Collector', 'SAC', 'push', 'sample', 'q_pack', 'sac_critic', 'sac_actor', 'q_action_grad', 'polyak',
           'push_reference', 'sample_index_reference', 'sample_word_reference', 'sample_reference', 'q_pack_reference', 'critic_reference',
           'actor_reference', 'action_grad_reference', 'polyak_reference', 'EbReplayPushArgs', 'EbReplaySampleArgs', 'EbQPackArgs',
           'EbSacCriticArgs', 'EbSacActorArgs', 'EbQActionGradArgs', 'EbPolyakSegment', 'EbPolyakArgs', 'EB_OFFPOLICY_ABI_VERSION',
           'EB_OFFPOLICY_MAX_OBS', 'EB_OFFPOLICY_MAX_ACT', 'EB_OFFPOLICY_ROWS', 'EB_OFFPOLICY_ALPHA_BLOCKS', 'EB_OFFPOLICY_MAX_SEGMENTS',
           'OFFPOLICY_PROTOTYPES', 'offpolicy_api']

_P, _I, _F, _U, _L = C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_int64
EB_OFFPOLICY_ABI_VERSION = 1
EB_OFFPOLICY_MAX_OBS = 4096
EB_OFFPOLICY_MAX_ACT = 16
EB_OFFPOLICY_ROWS = 32
EB_OFFPOLICY_ALPHA_BLOCKS = 64
EB_OFFPOLICY_MAX_SEGMENTS = 32
THREADS = 256                                                  # of every kernel (csrc/eb_offpolicy_device.h)
DONE_TIME_LIMIT = 7                                            # EB_DONE_TIME_LIMIT (include/envbuild.h)
HEADER = 'envbuild_offpolicy.h'
_f = np.float32
_QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


class EbReplayPushArgs(C.Structure):
    """eb_replay_push_args of include/envbuild_offpolicy.h"""
    _fields_ = [('capacity', _I), ('n', _I), ('start', _I), ('obs_dim', _I), ('act_dim', _I), ('fill_after', _I), ('obs', _P), ('act', _P),
                ('rew', _P), ('next_obs', _P), ('nonterminal', _P), ('fill', _P), ('prev_obs', _P), ('action', _P), ('reward', _P),
                ('obs_after', _P), ('done_code', _P), ('final_obs', _P), ('stream', _P)]


class EbReplaySampleArgs(C.Structure):
    """eb_replay_sample_args"""
    _fields_ = [('capacity', _I), ('m', _I), ('obs_dim', _I), ('act_dim', _I), ('obs', _P), ('act', _P), ('rew', _P), ('next_obs', _P),
                ('nonterminal', _P), ('fill', _P), ('seed', _U), ('draw', _U), ('counter', _P), ('indices', _P), ('index_bytes', _I),
                ('obs_out', _P), ('qin_out', _P), ('next_obs_out', _P), ('rew_out', _P), ('nonterminal_out', _P), ('index_out', _P),
                ('noise_id_out', _P), ('stream', _P)]


class EbQPackArgs(C.Structure):
    """eb_q_pack_args"""
    _fields_ = [('m', _I), ('obs_dim', _I), ('act_dim', _I), ('obs', _P), ('act', _P), ('qin', _P), ('stream', _P)]


class EbSacCriticArgs(C.Structure):
    """eb_sac_critic_args"""
    _fields_ = [('m', _I), ('q1t', _P), ('q2t', _P), ('logp_next', _P), ('rew', _P), ('nonterminal', _P), ('q1', _P), ('q2', _P),
                ('log_alpha', _P), ('alpha', _F), ('gamma', _F), ('reward_scale', _F), ('inv_m', _F), ('y', _P), ('loss1', _P),
                ('loss2', _P), ('g_q1', _P), ('g_q2', _P), ('stream', _P)]


class EbSacActorArgs(C.Structure):
    """eb_sac_actor_args"""
    _fields_ = [('m', _I), ('q1', _P), ('q2', _P), ('logp', _P), ('log_alpha', _P), ('alpha', _F), ('inv_m', _F), ('target_entropy', _F),
                ('loss', _P), ('g_q1', _P), ('g_q2', _P), ('g_logp', _P), ('g_log_alpha', _P), ('partials', _P), ('stream', _P)]


class EbQActionGradArgs(C.Structure):
    """eb_q_action_grad_args"""
    _fields_ = [('m', _I), ('obs_dim', _I), ('act_dim', _I), ('g_in1', _P), ('g_in2', _P), ('g_a', _P), ('stream', _P)]


class EbPolyakSegment(C.Structure):
    """eb_polyak_segment"""
    _fields_ = [('target', _P), ('online', _P), ('count', _L)]


class EbPolyakArgs(C.Structure):
    """eb_polyak_args"""
    _fields_ = [('n_segments', _I), ('segments', EbPolyakSegment * EB_OFFPOLICY_MAX_SEGMENTS), ('tau', _F), ('stream', _P)]


# include/envbuild_offpolicy.h: name -> (restype, argtypes) for every symbol the header declares
OFFPOLICY_PROTOTYPES = {
    'eb_offpolicy_abi_version': (C.c_int, []),
    'eb_offpolicy_last_error': (C.c_char_p, []),
    'eb_replay_push': (C.c_int, [C.POINTER(EbReplayPushArgs)]),
    'eb_replay_sample': (C.c_int, [C.POINTER(EbReplaySampleArgs)]),
    'eb_q_pack': (C.c_int, [C.POINTER(EbQPackArgs)]),
    'eb_sac_critic': (C.c_int, [C.POINTER(EbSacCriticArgs)]),
    'eb_sac_actor': (C.c_int, [C.POINTER(EbSacActorArgs)]),
    'eb_q_action_grad': (C.c_int, [C.POINTER(EbQActionGradArgs)]),
    'eb_polyak': (C.c_int, [C.POINTER(EbPolyakArgs)]),
}


class OffpolicyApi(object):
    """libenvbuild_offpolicy.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in OFFPOLICY_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in OFFPOLICY_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_offpolicy_abi_version()
        if v != EB_OFFPOLICY_ABI_VERSION:
            raise _capi.EbError('%s: offpolicy ABI version %d, expected %d (include/%s)' % (path, v, EB_OFFPOLICY_ABI_VERSION, HEADER))
        lib = self.lib
        self.push, self.sample, self.q_pack = lib.eb_replay_push, lib.eb_replay_sample, lib.eb_q_pack
        self.sac_critic, self.sac_actor, self.q_action_grad, self.polyak = lib.eb_sac_critic, lib.eb_sac_actor, lib.eb_q_action_grad, lib.eb_polyak

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_offpolicy_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(offpolicy): %s' % msg)
            raise _capi.EbError('envbuild(offpolicy) error %d: %s' % (rc, msg))


_offpolicy_api = None


def offpolicy_api():
    """The off-policy library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls
    back — when it is absent or was built from other sources and cannot be rebuilt."""
    global _offpolicy_api
    if _offpolicy_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.offpolicy_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.OFFPOLICY_LIB, _build.CSRC))
            try:
                _build.build_offpolicy()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.OFFPOLICY_LIB, e))
        _offpolicy_api = OffpolicyApi(_build.OFFPOLICY_LIB)
    return _offpolicy_api


def _ptr(t):
    return None if t is None else t.data_ptr()


_dev = _collect._dev


def _f32(t, what, shape, device):
    return None if t is None else _dev(t, what, np.float32, shape, device)


def _issue(fn_name, a, device):
    api = offpolicy_api()
    with torch.cuda.device(device):
        a.stream = _stream(device)
        api.check(getattr(api, fn_name)(C.byref(a)))


def _dims(D, A):
    D, A = int(D), int(A)
    if not 1 <= D <= EB_OFFPOLICY_MAX_OBS:
        raise ValueError('obs_dim must be in 1 .. %d, got %d' % (EB_OFFPOLICY_MAX_OBS, D))
    if not 1 <= A <= EB_OFFPOLICY_MAX_ACT:
        raise ValueError('act_dim must be in 1 .. %d, got %d' % (EB_OFFPOLICY_MAX_ACT, A))
    return D, A


# ---- the ring ---------------------------------------------------------------------------------------------------------------------------
class ReplayBuffer(object):
    """The ring of include/envbuild_offpolicy.h on the device — obs [C, D], act [C, A], rew [C], next_obs [C, D], nonterminal [C] and the
    8-byte word `fill` — and its cursor on the host.  push() writes a batch at the cursor and moves it; `len(buffer)` is the host's view of
    fill (no device read).  sample_into() draws a minibatch into preallocated outputs; the kernel reads *fill itself."""

    def __init__(self, capacity, obs_dim, act_dim, device=None):
        from .dynamics_and_models import _resolve_device
        C_, (D, A) = int(capacity), _dims(obs_dim, act_dim)
        if C_ < 1 or C_ * (D + A) > 2 ** 31 - 1:
            raise ValueError('capacity must be at least 1 with capacity * (obs_dim + act_dim) <= 2^31 - 1, got %d' % C_)
        self.capacity, self.obs_dim, self.act_dim, self.device = C_, D, A, _resolve_device(device)
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.obs, self.act, self.rew, self.next_obs, self.nonterminal = new(C_, D), new(C_, A), new(C_), new(C_, D), new(C_)
        self.fill = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self.cursor, self.size = 0, 0

    def __len__(self):
        return self.size

    def ring(self):
        """the five arrays as a dict of NumPy copies (what the restatements work on)"""
        return {k: getattr(self, k).cpu().numpy().copy() for k in ('obs', 'act', 'rew', 'next_obs', 'nonterminal')}

    def push_args(self, n):
        """eb_replay_push_args for a batch of n rows with the ring's pointers set; the sources, start and fill_after are set per call"""
        return EbReplayPushArgs(capacity=self.capacity, n=int(n), obs_dim=self.obs_dim, act_dim=self.act_dim, obs=_ptr(self.obs),
                                act=_ptr(self.act), rew=_ptr(self.rew), next_obs=_ptr(self.next_obs), nonterminal=_ptr(self.nonterminal),
                                fill=_ptr(self.fill))

    def advance(self, n):
        """the host's bookkeeping of a completed batch of n rows -> (start it was written at, fill after it)"""
        start = self.cursor
        self.cursor = (self.cursor + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
        return start, self.size

    def push(self, prev_obs, action, reward, obs_after, done_code, final_obs=None):
        """one batch of n transitions at the cursor: ONE launch on the current stream.  Every argument is a device tensor."""
        n = reward.numel()
        if n > self.capacity:
            raise ValueError('a batch of %d rows does not fit a ring of %d' % (n, self.capacity))
        dev, D, A = self.device, self.obs_dim, self.act_dim
        _f32(prev_obs, 'prev_obs', (n, D), dev), _f32(action, 'action', (n, A), dev), _f32(obs_after, 'obs_after', (n, D), dev)
        _f32(final_obs, 'final_obs', (n, D), dev), _dev(reward, 'reward', device=dev), _dev(done_code, 'done_code', np.uint8, (n,), dev)
        a = self.push_args(n)
        a.start = self.cursor
        a.fill_after = min(self.size + n, self.capacity)
        a.prev_obs, a.action, a.reward, a.obs_after = _ptr(prev_obs), _ptr(action), _ptr(reward), _ptr(obs_after)
        a.done_code, a.final_obs = _ptr(done_code), _ptr(final_obs)
        _issue('push', a, dev)
        self.advance(n)

    def sample_args(self, batch, seed=0, draw=0, counter=None, indices=None):
        """eb_replay_sample_args over this ring into the tensors of `batch` (a dict or an object with obs, qin, next_obs, rew,
        nonterminal, index, noise_id: each optional)"""
        get = batch.get if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        outs = {k: get(k) for k in ('obs', 'qin', 'next_obs', 'rew', 'nonterminal', 'index', 'noise_id')}
        given = [t for t in outs.values() if t is not None]
        if not given:
            raise ValueError('sample_into needs at least one output')
        m, dev, D, A = given[0].shape[0], self.device, self.obs_dim, self.act_dim
        _f32(outs['obs'], 'obs', (m, D), dev), _f32(outs['qin'], 'qin', (m, D + A), dev), _f32(outs['next_obs'], 'next_obs', (m, D), dev)
        _f32(outs['rew'], 'rew', (m,), dev), _f32(outs['nonterminal'], 'nonterminal', (m,), dev)
        if outs['index'] is not None:
            _dev(outs['index'], 'index', np.int32, (m,), dev)
        if outs['noise_id'] is not None:
            _dev(outs['noise_id'], 'noise_id', np.int32, (m,), dev)
        a = EbReplaySampleArgs(capacity=self.capacity, m=m, obs_dim=D, act_dim=A, obs=_ptr(self.obs), act=_ptr(self.act), rew=_ptr(self.rew),
                               next_obs=_ptr(self.next_obs), nonterminal=_ptr(self.nonterminal), fill=_ptr(self.fill),
                               seed=int(seed) & (2 ** 64 - 1), draw=int(draw) & (2 ** 64 - 1), counter=_ptr(counter),
                               obs_out=_ptr(outs['obs']), qin_out=_ptr(outs['qin']), next_obs_out=_ptr(outs['next_obs']),
                               rew_out=_ptr(outs['rew']), nonterminal_out=_ptr(outs['nonterminal']), index_out=_ptr(outs['index']),
                               noise_id_out=_ptr(outs['noise_id']))
        if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
            raise TypeError('counter must be a device int64 tensor of one element')
        if indices is not None:
            if not (isinstance(indices, torch.Tensor) and indices.is_cuda and indices.is_contiguous() and indices.shape == (m,)
                    and indices.dtype in (torch.int32, torch.int64)):
                raise TypeError('indices must be a contiguous int32 or int64 device tensor of %d elements' % m)
            a.indices, a.index_bytes = _ptr(indices), indices.element_size()
        return a

    def sample_into(self, batch, seed=0, draw=0, counter=None, indices=None):
        """eb_replay_sample: ONE launch on the current stream.  Keyed by (seed, *counter + draw), or the explicit `indices`."""
        _issue('sample', self.sample_args(batch, seed, draw, counter, indices), self.device)


def push(buffer, prev_obs, action, reward, obs_after, done_code, final_obs=None):
    """eb_replay_push at the buffer's cursor (ReplayBuffer.push)"""
    buffer.push(prev_obs, action, reward, obs_after, done_code, final_obs)


def sample(buffer, batch, seed=0, draw=0, counter=None, indices=None):
    """eb_replay_sample (ReplayBuffer.sample_into)"""
    buffer.sample_into(batch, seed, draw, counter, indices)


# ---- the elementwise entries ----------------------------------------------------------------------------------------------------------------
def _pack_args(qin, obs=None, act=None):
    m, W = qin.shape
    given = obs if obs is not None else act
    if given is None:
        raise ValueError('q_pack needs obs, act or both')
    D = obs.shape[1] if obs is not None else W - act.shape[1]
    A = W - D
    dev = qin.device
    _f32(qin, 'qin', (m, W), dev), _f32(obs, 'obs', (m, D), dev), _f32(act, 'act', (m, A), dev)
    return EbQPackArgs(m=m, obs_dim=D, act_dim=A, obs=_ptr(obs), act=_ptr(act), qin=_ptr(qin))


def q_pack(qin, obs=None, act=None):
    """eb_q_pack: qin [m, D + A]; qin[:, :D] = obs when given, qin[:, D:] = act when given.  ONE launch."""
    _issue('q_pack', _pack_args(qin, obs, act), qin.device)
    return qin


def _alpha(a, alpha, log_alpha, device):
    if log_alpha is not None:
        a.log_alpha = _ptr(_f32(log_alpha, 'log_alpha', (1,), device))
    elif alpha is None:
        raise ValueError('pass alpha by value or log_alpha on the device')
    else:
        a.alpha = float(alpha)


def _critic_args(q1t, q2t, logp_next, rew, nonterminal, q1=None, q2=None, alpha=None, log_alpha=None, gamma=0.99, reward_scale=1.0,
                 inv_m=None, y=None, loss1=None, loss2=None, g_q1=None, g_q2=None):
    m, dev = q1t.numel(), q1t.device
    for name, t in (('q1t', q1t), ('q2t', q2t), ('logp_next', logp_next), ('rew', rew), ('nonterminal', nonterminal), ('q1', q1), ('q2', q2),
                    ('y', y), ('loss1', loss1), ('loss2', loss2), ('g_q1', g_q1), ('g_q2', g_q2)):
        if t is not None and (_dev(t, name, device=dev).numel() != m):
            raise ValueError('%s must hold %d values' % (name, m))
    a = EbSacCriticArgs(m=m, q1t=_ptr(q1t), q2t=_ptr(q2t), logp_next=_ptr(logp_next), rew=_ptr(rew), nonterminal=_ptr(nonterminal),
                        q1=_ptr(q1), q2=_ptr(q2), gamma=float(gamma), reward_scale=float(reward_scale),
                        inv_m=float(_f(1) / _f(m)) if inv_m is None else float(inv_m), y=_ptr(y), loss1=_ptr(loss1), loss2=_ptr(loss2),
                        g_q1=_ptr(g_q1), g_q2=_ptr(g_q2))
    _alpha(a, alpha, log_alpha, dev)
    return a


def sac_critic(q1t, q2t, logp_next, rew, nonterminal, **kw):
    """eb_sac_critic: the TD target and both critics' loss rows and cotangents.  ONE launch.  Keywords: q1, q2, alpha | log_alpha, gamma,
    reward_scale, inv_m (1 / m), and the outputs y, loss1, loss2, g_q1, g_q2."""
    _issue('sac_critic', _critic_args(q1t, q2t, logp_next, rew, nonterminal, **kw), q1t.device)


def _actor_args(q1, q2, logp, alpha=None, log_alpha=None, inv_m=None, target_entropy=0.0, loss=None, g_q1=None, g_q2=None, g_logp=None,
                g_log_alpha=None, partials=None):
    m, dev = q1.numel(), q1.device
    for name, t in (('q1', q1), ('q2', q2), ('logp', logp), ('loss', loss), ('g_q1', g_q1), ('g_q2', g_q2), ('g_logp', g_logp)):
        if t is not None and (_dev(t, name, device=dev).numel() != m):
            raise ValueError('%s must hold %d values' % (name, m))
    if g_log_alpha is not None:
        _f32(g_log_alpha, 'g_log_alpha', (1,), dev)
        _dev(partials, 'partials', np.float64, (EB_OFFPOLICY_ALPHA_BLOCKS,), dev)
    a = EbSacActorArgs(m=m, q1=_ptr(q1), q2=_ptr(q2), logp=_ptr(logp), inv_m=float(_f(1) / _f(m)) if inv_m is None else float(inv_m),
                       target_entropy=float(target_entropy), loss=_ptr(loss), g_q1=_ptr(g_q1), g_q2=_ptr(g_q2), g_logp=_ptr(g_logp),
                       g_log_alpha=_ptr(g_log_alpha), partials=_ptr(partials) if g_log_alpha is not None else None)
    _alpha(a, alpha, log_alpha, dev)
    return a


def sac_actor(q1, q2, logp, **kw):
    """eb_sac_actor: the actor loss rows and the cotangents of q1, q2 and logp; with g_log_alpha (and partials, float64 [64]) the
    temperature gradient too.  ONE launch, TWO with g_log_alpha."""
    _issue('sac_actor', _actor_args(q1, q2, logp, **kw), q1.device)


def _action_grad_args(g_in1, g_in2, g_a):
    m, W = g_in1.shape
    A = g_a.shape[1]
    dev = g_in1.device
    _f32(g_in1, 'g_in1', (m, W), dev), _f32(g_in2, 'g_in2', (m, W), dev), _f32(g_a, 'g_a', (m, A), dev)
    return EbQActionGradArgs(m=m, obs_dim=W - A, act_dim=A, g_in1=_ptr(g_in1), g_in2=_ptr(g_in2), g_a=_ptr(g_a))


def q_action_grad(g_in1, g_in2, g_a):
    """eb_q_action_grad: g_a [m, A] = g_in1[:, D:] + g_in2[:, D:] (g_in2 None: one critic).  ONE launch."""
    _issue('q_action_grad', _action_grad_args(g_in1, g_in2, g_a), g_in1.device)
    return g_a


def _polyak_args(pairs, tau):
    pairs = list(pairs)
    if len(pairs) > EB_OFFPOLICY_MAX_SEGMENTS:
        raise ValueError('polyak takes at most %d segments, got %d' % (EB_OFFPOLICY_MAX_SEGMENTS, len(pairs)))
    a = EbPolyakArgs(n_segments=len(pairs), tau=float(tau))
    for k, (target, online) in enumerate(pairs):
        _dev(target, 'target'), _dev(online, 'online', shape=tuple(target.shape), device=target.device)
        seg = a.segments[k]
        seg.target, seg.online, seg.count = _ptr(target), _ptr(online), target.numel()
    return a


def polyak(pairs, tau):
    """eb_polyak: target = fmaf(tau, online - target, target) over up to 32 (target, online) pairs of device tensors.  ONE launch."""
    pairs = list(pairs)
    if pairs:
        _issue('polyak', _polyak_args(pairs, tau), pairs[0][0].device)


# ---- the contract in NumPy ------------------------------------------------------------------------------------------------------------------
def push_reference(ring, start, prev_obs=None, action=None, reward=None, obs_after=None, done_code=None, final_obs=None):
    """eb_replay_push on a dict of NumPy arrays (obs, act, rew, next_obs, nonterminal), in place: row i goes to slot (start + i) mod C.
    The before part with prev_obs / action, the after part with reward / obs_after / done_code (/ final_obs)."""
    C_ = ring['rew'].shape[0]
    n = len(prev_obs) if prev_obs is not None else len(reward)
    slots = (int(start) + np.arange(n, dtype=np.int64)) % C_
    if prev_obs is not None:
        ring['obs'][slots] = np.asarray(prev_obs, _f)
        ring['act'][slots] = np.asarray(action, _f)
    if reward is not None:
        c = np.asarray(done_code, np.uint8).reshape(n)
        nxt = np.asarray(obs_after, _f).copy()
        if final_obs is not None:
            nxt[c != 0] = np.asarray(final_obs, _f)[c != 0]
        ring['next_obs'][slots] = nxt
        ring['rew'][slots] = np.asarray(reward, _f).reshape(n)
        ring['nonterminal'][slots] = np.where((c == 0) | ((c == DONE_TIME_LIMIT) & (final_obs is not None)), _f(1), _f(0))
    return ring


def _mulhi64(w, f):
    """the high half of the 128-bit product of uint64 words w and f < 2^32, in uint64 pieces"""
    f = np.uint64(f)
    hi, lo = w >> np.uint64(32), w & np.uint64(0xFFFFFFFF)
    return (hi * f + ((lo * f) >> np.uint64(32))) >> np.uint64(32)


def sample_word_reference(m, seed, draw, base=0):
    """w(r) for r = 0 .. m - 1 under key = splitmix64(seed + GOLDEN * (base + draw)): uint64 [m]"""
    with np.errstate(over='ignore'):
        key = _splitmix64(np.array([int(seed) % 2 ** 64], np.uint64) + _GOLDEN * np.array([(int(base) + int(draw)) % 2 ** 64], np.uint64))
        return _splitmix64(key + _GOLDEN * np.arange(int(m), dtype=np.uint64))


def sample_index_reference(m, f, seed, draw, base=0):
    """the keyed route's indices: j(r) = mulhi64(w(r), f) in [0, f) -> int64 [m]; all -1 with f == 0"""
    f = int(f)
    if f <= 0:
        return np.full(int(m), -1, np.int64)
    with np.errstate(over='ignore'):
        return _mulhi64(sample_word_reference(m, seed, draw, base), f).astype(np.int64)


def sample_reference(ring, f, m, seed=0, draw=0, base=0, indices=None):
    """eb_replay_sample on a dict of NumPy arrays -> dict(obs, qin, next_obs, rew, nonterminal, index, noise_id).  f: the fill word."""
    C_ = ring['rew'].shape[0]
    f = min(max(int(f), 0), C_)
    if indices is None:
        idx = sample_index_reference(m, f, seed, draw, base)
    else:
        idx = np.asarray(indices).astype(np.int64).reshape(m)
        idx = np.where((idx >= 0) & (idx < f), idx, -1)
    ok = idx >= 0
    at = np.where(ok, idx, 0)

    def take(a):
        out = np.asarray(a, _f)[at].copy()
        out[~ok] = _QNAN
        return out
    obs = take(ring['obs'])
    return dict(obs=obs, qin=np.concatenate([obs, take(ring['act'])], axis=1), next_obs=take(ring['next_obs']), rew=take(ring['rew']),
                nonterminal=take(ring['nonterminal']), index=idx.astype(np.int32),
                noise_id=(sample_word_reference(m, seed, draw, base) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def q_pack_reference(qin, obs=None, act=None):
    """eb_q_pack on NumPy arrays, in place -> qin"""
    if obs is not None:
        qin[:, :obs.shape[1]] = obs
    if act is not None:
        qin[:, qin.shape[1] - act.shape[1]:] = act
    return qin


def _min_nan(a, b):
    """the kernels' minimum: m = b < a ? b : a; m = b != b ? b : m — a NaN in either travels"""
    m = np.where(b < a, b, a)
    return np.where(b != b, b, m).astype(_f)


def _alpha_of(alpha, log_alpha):
    return _exp_det(np.asarray([log_alpha], _f))[0] if log_alpha is not None else _f(alpha)


def critic_reference(q1t, q2t, logp_next, rew, nonterminal, q1, q2, alpha=None, log_alpha=None, gamma=0.99, reward_scale=1.0, inv_m=None):
    """eb_sac_critic in NumPy, one fp32 rounding per line and the single-rounding fmaf where the contract has it ->
    dict(y, loss1, loss2, g_q1, g_q2)"""
    q1t, q2t, logp_next, rew, nonterminal, q1, q2 = (np.asarray(x, _f).reshape(-1) for x in (q1t, q2t, logp_next, rew, nonterminal, q1, q2))
    inv_m = _f(1) / _f(len(q1t)) if inv_m is None else _f(inv_m)
    with np.errstate(all='ignore'):
        a = _alpha_of(alpha, log_alpha)
        qm = _min_nan(q1t, q2t)
        e = a * logp_next
        v = qm - e
        y = _fmaf(_f(gamma) * nonterminal, v, _f(reward_scale) * rew)
        d1, d2 = q1 - y, q2 - y
        return dict(y=y, loss1=(_f(0.5) * d1) * d1, loss2=(_f(0.5) * d2) * d2, g_q1=d1 * inv_m, g_q2=d2 * inv_m)


def actor_reference(q1, q2, logp, alpha=None, log_alpha=None, inv_m=None, target_entropy=None):
    """eb_sac_actor in NumPy -> dict(loss, g_q1, g_q2, g_logp) and, with target_entropy, partials (float64 [64]) and g_log_alpha
    (float32 [1]) in the kernels' order: lane t of block b over the rows b * 256 + t + k * 16384, the block by halving, the 64 ascending"""
    q1, q2, logp = (np.asarray(x, _f).reshape(-1) for x in (q1, q2, logp))
    m = len(q1)
    inv_m = _f(1) / _f(m) if inv_m is None else _f(inv_m)
    with np.errstate(all='ignore'):
        a = _alpha_of(alpha, log_alpha)
        first = q1 <= q2
        out = dict(loss=(a * logp) - _min_nan(q1, q2), g_q1=np.where(first, -inv_m, _f(0)).astype(_f),
                   g_q2=np.where(first, _f(0), -inv_m).astype(_f), g_logp=np.full(m, a * inv_m, _f))
        if target_entropy is not None:
            B, T = EB_OFFPOLICY_ALPHA_BLOCKS, THREADS
            passes = -(-m // (B * T))
            terms = np.zeros(passes * B * T, np.float64)
            terms[:m] = logp.astype(np.float64) + np.float64(_f(target_entropy))
            valid = (np.arange(passes * B * T) < m).reshape(passes, B, T)
            terms = terms.reshape(passes, B, T)
            lane = np.zeros((B, T), np.float64)
            for k in range(passes):
                lane = np.where(valid[k], lane + terms[k], lane)
            w = T // 2
            while w:
                lane[:, :w] = lane[:, :w] + lane[:, w:2 * w]
                w //= 2
            partials = lane[:, 0].copy()
            S = np.float64(0)
            for b in range(B):
                S = S + partials[b]
            out['partials'] = partials
            out['g_log_alpha'] = np.array([-(S / np.float64(m))], np.float64).astype(_f)
    return out


def action_grad_reference(g_in1, g_in2, act_dim):
    """eb_q_action_grad in NumPy: the last act_dim columns of g_in1 (+ g_in2's), one fp32 addition -> [m, act_dim]"""
    a = np.asarray(g_in1, _f)[:, -int(act_dim):]
    with np.errstate(all='ignore'):
        return np.ascontiguousarray(a if g_in2 is None else a + np.asarray(g_in2, _f)[:, -int(act_dim):])


def polyak_reference(target, online, tau):
    """eb_polyak in NumPy: fmaf(tau, online - target, target) -> a new float32 array"""
    target, online = np.asarray(target, _f), np.asarray(online, _f)
    with np.errstate(all='ignore'):
        return _fmaf(_f(tau), online - target, target)


# ---- the collector ----------------------------------------------------------------------------------------------------------------------------
class Collector(object):
    """One env step of B envs into a ReplayBuffer, everything a library launch on the current stream:

        step():          eb_policy_sample(env's observation -> actions; counter = the step number)        (1 kernel)
                         env.step(actions)                                                               (eb_env_step)
                         eb_replay_push(both parts: the observation acted on, the action, the step's outputs)   (1 kernel)
        random_steps(k): the same with eb_policy_sample_from_logits on zero logits (mean 0, log-std 0: a tanh-squashed standard normal
                         scaled by action_range) in place of the policy — the warm-up's documented equivalent of uniform actions, from
                         the same counter-based noise

    THREE launches per env step.  `env`: a CrossroadEnd2end with auto_reset=True, copy_outputs=False and n_env > 1.  With copy_outputs=False
    the env writes each step's observation into the other of two buffer sets (endtoend.py: _step_buffers), so the observation the policy
    acted on is still intact behind env.step and ONE push carries both parts.  The exception is the first step after a reset that wrote
    into the set the step is about to use (the env then moves its input aside): there step() pushes the before part in front of env.step
    and the after part behind it — FOUR launches, once.  A finished env's transition ends in info['final_observation']'s row.  step()
    makes no torch operation, no allocation and no host read.  The collection is issued eagerly: CrossroadEnd2end.step passes its respawn
    and reset counters by value, and the ring's cursor lives on the host."""

    def __init__(self, env, policy, buffer, action_range, seed=0):
        from . import policy_sample
        from .endtoend import CrossroadEnd2end
        from .policy import MLPNet
        if not isinstance(env, CrossroadEnd2end):
            raise TypeError('Collector drives a CrossroadEnd2end, got %s' % type(env).__name__)
        if not env.auto_reset or env.copy_outputs or env.n_env < 2:
            raise ValueError('Collector needs an env with auto_reset=True, copy_outputs=False and n_env > 1')
        if not isinstance(policy, MLPNet):
            raise TypeError('policy must be an MLPNet')
        B, D, A = env.n_env, env.obs_dim, env.action_number
        if policy.input_dim != D or policy.output_dim != 2 * A or policy.device != env.device:
            raise ValueError('the policy must map %d -> %d on the device of the env' % (D, 2 * A))
        if not policy_sample._supported(policy):
            raise ValueError('Collector: eb_policy_sample_supported refuses the policy %s (precision %r)' % (policy.name, policy.precision))
        if (buffer.obs_dim, buffer.act_dim, buffer.device) != (D, A, env.device) or buffer.capacity < B:
            raise ValueError('the buffer must hold rows of %d + %d floats on the device of the env, at least %d of them' % (D, A, B))
        self.env, self.policy, self.buffer, self.device = env, policy, buffer, env.device
        self.n_env, self.obs_dim, self.act_dim = B, D, A
        self.action_range, self.seed, self.steps = policy_sample._range(action_range), int(seed) & ((1 << 64) - 1), 0
        self.actions = torch.zeros((B, A), dtype=torch.float32, device=self.device)
        self.zero_logits = torch.zeros((B, 2 * A), dtype=torch.float32, device=self.device)
        self.api = offpolicy_api()
        fns = policy_sample.bind(policy.api)
        self._sample, self._from_logits = fns['eb_policy_sample'], fns['eb_policy_sample_from_logits']
        self._push = buffer.push_args(B)
        self._last_obs = None                                     # the observation buffer the last step() handed out

    def _step(self, random):
        env, pol, buf, B, s = self.env, self.policy, self.buffer, self.n_env, None
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            prev = env.obs.t
            if random:
                pol.api.check(self._from_logits(B, 2 * self.act_dim, self.zero_logits.data_ptr(), None, None, self.seed, self.steps,
                                                self.action_range, self.actions.data_ptr(), None, None, s))
            else:
                pol.api.check(self._sample(pol._handle, B, prev.data_ptr(), None, None, self.seed, self.steps, self.action_range,
                                           self.actions.data_ptr(), None, None, None, s))
            a = self._push
            a.start, a.stream = buf.cursor, s
            a.fill_after = min(buf.size + B, buf.capacity)
            split = self._last_obs is None or prev.data_ptr() != self._last_obs      # someone reset the env since our last step
            if split:
                a.prev_obs, a.action, a.reward, a.obs_after, a.done_code, a.final_obs = prev.data_ptr(), self.actions.data_ptr(), None, None, None, None
                self.api.check(self.api.push(C.byref(a)))
            obs, reward, _done, info = env.step(self.actions)
            a.reward, a.obs_after, a.done_code = reward.t.data_ptr(), obs.t.data_ptr(), env.done_code.data_ptr()
            a.final_obs = info['final_observation'].t.data_ptr()
            if split:
                a.prev_obs, a.action = None, None
            else:
                a.prev_obs, a.action = prev.data_ptr(), self.actions.data_ptr()
            self.api.check(self.api.push(C.byref(a)))
            buf.advance(B)
            self._last_obs = obs.t.data_ptr()
        self.steps += 1

    def step(self):
        """one env step with the policy's actions, pushed"""
        self._step(False)

    def random_steps(self, k):
        """k env steps with the warm-up's actions, pushed"""
        for _ in range(int(k)):
            self._step(True)


# ---- one SAC update -----------------------------------------------------------------------------------------------------------------------------
class _Buffers(object):
    def __init__(self, **tensors):
        self.__dict__.update(tensors)


class SAC(object):
    """One soft actor-critic update of `batch` rows for a policy and two critic `TrainableMLPNet`s as a fixed chain of launches on the
    current stream (the number of each entry's kernels in brackets; an eb_mlp_backward is 3 kernels with g_params and 1 with g_obs alone):

         1  eb_replay_sample            mb.obs, mb.qin = [obs | act], mb.next_obs, mb.rew, mb.nonterminal, mb.noise_id         (1)
         2  eb_policy_sample(next_obs)  a', logp' under the noise of mb.noise_id, counter 0                                    (1)
            eb_q_pack                   qin_next = [next_obs | a']                                                             (1)
         3  eb_mlp_forward x 4          the target critics on qin_next, the online critics on mb.qin                           (4)
         4  eb_sac_critic               y, loss1, loss2 and the critics' cotangents                                            (1)
         5  eb_mlp_backward x 2         into the critics' flat gradients                                                       (2 x 3)
         6  eb_adam_step x 2, eb_mlp_set_params_device x 2                                                                     (2 x 2 + 2)
         7  eb_policy_sample(obs)       a_new, logp with eps_out and logits_out, counter 1                                     (1)
            eb_q_pack                   mb.qin's action columns = a_new                                                        (1)
         8  eb_mlp_forward x 2          the UPDATED critics at [obs | a_new] — eb_sac_actor's select needs their values —      (2)
         9  eb_sac_actor                the actor loss rows, the cotangents of q1, q2 and logp, the temperature gradient       (2)
            eb_mlp_backward x 2         the critics' g_obs alone                                                               (2 x 1)
        10  eb_q_action_grad            dQ/da [batch, A]                                                                       (1)
        11  eb_policy_sample_vjp        the cotangent of the logits                                                            (1)
        12  eb_mlp_backward(policy)     into the policy's flat gradient                                                        (3)
        13  eb_adam_step x 2            the policy, log_alpha;  eb_mlp_set_params_device(policy)                               (2 x 2 + 1)
        14  eb_polyak                   both target tensors, one launch;  eb_mlp_set_params_device x 2 on the target handles;
            eb_epoch_advance            the draw counter                                                                       (1 + 2 + 1)

    The target critics are plain `MLPNet` handles refilled from the Polyak-averaged flat tensors `target_flat`.  The action noise of a
    replayed graph comes from device state alone: eb_replay_sample's noise_id_out is eb_policy_sample's row_ids.  Everything is
    allocated here, once.  step() makes no torch arithmetic, no host read, no allocation and no autograd.  KERNELS is the number of
    kernel nodes of capture()'s graph."""

    KERNELS = 42

    def __init__(self, policy, q1, q2, buffer, batch, gamma=0.99, tau=0.005, lr=3e-4, lr_q=None, lr_alpha=None, target_entropy=None,
                 log_alpha0=0.0, reward_scale=1.0, action_range=1.0, seed=0, betas=(0.9, 0.999), eps=1e-8):
        from . import epoch, policy_sample, train
        from .policy import MLPNet
        from .policy_grad import TrainableMLPNet
        for net in (policy, q1, q2):
            if not isinstance(net, TrainableMLPNet):
                raise TypeError('SAC trains TrainableMLPNets, got %s' % type(net).__name__)
        D, A, n, dev = buffer.obs_dim, buffer.act_dim, int(batch), buffer.device
        if n < 1:
            raise ValueError('batch must be at least 1')
        if (policy.input_dim, policy.output_dim) != (D, 2 * A) or any((q.input_dim, q.output_dim) != (D + A, 1) for q in (q1, q2)):
            raise ValueError('the policy must map %d -> %d and the critics %d -> 1' % (D, 2 * A, D + A))
        if any(net.device != dev for net in (policy, q1, q2)):
            raise ValueError('the networks must live on the device of the buffer')
        if not policy_sample._supported(policy):
            policy.api.check(-1)
        for name, v in (('gamma', gamma), ('tau', tau), ('reward_scale', reward_scale), ('log_alpha0', log_alpha0)):
            if not np.isfinite(v):
                raise ValueError('%s must be finite, got %r' % (name, v))
        self.policy, self.q1, self.q2, self.buffer, self.n, self.device, self.api = policy, q1, q2, buffer, n, dev, policy.api
        self.gamma, self.tau, self.reward_scale = float(gamma), float(tau), float(reward_scale)
        self.target_entropy = float(-A if target_entropy is None else target_entropy)
        self.action_range, self.seed = policy_sample._range(action_range), int(seed) & ((1 << 64) - 1)
        self.inv_m = float(_f(1) / _f(n))
        f32 = torch.float32
        new = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        self.mb = _Buffers(obs=new(n, D), qin=new(n, D + A), next_obs=new(n, D), rew=new(n), nonterminal=new(n),
                           noise_id=torch.zeros((n,), dtype=torch.int32, device=dev))
        self.rows = _Buffers(a_next=new(n, A), logp_next=new(n), qin_next=new(n, D + A), q1t=new(n), q2t=new(n), q1=new(n), q2=new(n),
                             y=new(n), loss1=new(n), loss2=new(n), g_q1=new(n), g_q2=new(n), a_new=new(n, A), logp=new(n),
                             logits=new(n, 2 * A), eps=new(n, A), q1n=new(n), q2n=new(n), aloss=new(n), ga_q1=new(n), ga_q2=new(n),
                             g_logp=new(n), g_in1=new(n, D + A), g_in2=new(n, D + A), g_a=new(n, A), g_logits=new(n, 2 * A))
        self.log_alpha = torch.full((1,), float(log_alpha0), dtype=f32, device=dev)
        self.g_log_alpha = new(1)
        self.partials = torch.zeros((EB_OFFPOLICY_ALPHA_BLOCKS,), dtype=torch.float64, device=dev)
        self.counter = torch.zeros((1,), dtype=torch.int64, device=dev)
        lr_q = lr if lr_q is None else lr_q
        lr_alpha = lr if lr_alpha is None else lr_alpha
        kw = dict(betas=betas, eps=eps)
        self.adam_q1, self.adam_q2 = train.Adam([q1], lr=lr_q, **kw), train.Adam([q2], lr=lr_q, **kw)
        self.adam_pi, self.adam_alpha = train.Adam([policy], lr=lr, **kw), train.Adam([self.log_alpha], lr=lr_alpha, **kw)
        seg = self.adam_alpha._args.segments[0]
        seg.grads, seg.count = _ptr(self.g_log_alpha), 1
        # the targets: plain inference handles over Polyak-averaged copies of the critics' flat tensors
        self.targets, self.target_flat = [], []
        for q in (q1, q2):
            q._sync()
            t = MLPNet(q.input_dim, q.num_hidden_layers, q.num_hidden_units, q.hidden_activation, 1, output_activation=q.output_activation,
                       device=dev, name=q.name + '_target')
            if q._obs_scale is not None:
                t.set_obs_scale(q._obs_scale)                     # (rebuilds the handle: before the weights go in)
            flat = q._flat.detach().clone()
            self.api.mlp_set_params_device(t._handle, C.c_void_p(flat.data_ptr()), _stream(dev))
            self.targets.append(t)
            self.target_flat.append(flat)
        policy._sync()
        self._ws = {}
        for net in (policy, q1, q2):
            need = C.c_size_t(0)
            self.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
            self._ws[net] = (torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value)
        fns = policy_sample.bind(self.api)
        self._sample, self._vjp = fns['eb_policy_sample'], fns['eb_policy_sample_vjp']
        self.off, self._epoch = offpolicy_api(), epoch.epoch_api()
        r, mb = self.rows, self.mb
        self._a_sample = buffer.sample_args(mb, seed=self.seed, draw=0, counter=self.counter)
        self._a_pack_next = _pack_args(r.qin_next, mb.next_obs, r.a_next)
        self._a_critic = _critic_args(r.q1t, r.q2t, r.logp_next, mb.rew, mb.nonterminal, q1=r.q1, q2=r.q2, log_alpha=self.log_alpha,
                                      gamma=self.gamma, reward_scale=self.reward_scale, inv_m=self.inv_m, y=r.y, loss1=r.loss1,
                                      loss2=r.loss2, g_q1=r.g_q1, g_q2=r.g_q2)
        self._a_pack_new = _pack_args(mb.qin, None, r.a_new)
        self._a_actor = _actor_args(r.q1n, r.q2n, r.logp, log_alpha=self.log_alpha, inv_m=self.inv_m, target_entropy=self.target_entropy,
                                    loss=r.aloss, g_q1=r.ga_q1, g_q2=r.ga_q2, g_logp=r.g_logp, g_log_alpha=self.g_log_alpha,
                                    partials=self.partials)
        self._a_grad = _action_grad_args(r.g_in1, r.g_in2, r.g_a)
        self._a_polyak = _polyak_args(zip(self.target_flat, (q1._flat, q2._flat)), self.tau)
        self._a_advance = epoch.EbEpochAdvanceArgs(counter=_ptr(self.counter), by=1)
        self._log = torch.zeros((7, n), dtype=f32, device=dev)

    def _backward(self, net, x, g_out, g_obs, g_params, s):
        ws, need = self._ws[net]
        self.api.mlp_backward(net._h, self.n, x.data_ptr(), g_out.data_ptr(), 0, 0.0, ws.data_ptr(), need, None, _ptr(g_obs), _ptr(g_params), s)

    def _upload(self, net, s):
        self.api.mlp_set_params_device(net._h, net._flat.data_ptr(), s)
        net._uploaded = net._flat._version

    def _draw(self, s):
        """step 1 of the chain: the minibatch into self.mb (a subclass draws it another way: env_build_amd.per.SAC)"""
        self.off.check(self.off.sample(C.byref(self._a_sample)))

    def _after_critic(self, s):
        """between eb_sac_critic and the critics' backward passes: nothing here (env_build_amd.per.SAC weighs the cotangents)"""

    def step(self):
        """the chain, on the current stream"""
        pol, q1, q2, api, off, n, r, mb = self.policy, self.q1, self.q2, self.api, self.off, self.n, self.rows, self.mb
        for net in (pol, q1, q2):
            net._sync()
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            ids = mb.noise_id.data_ptr()
            for a in (self._a_sample, self._a_pack_next, self._a_critic, self._a_pack_new, self._a_actor, self._a_grad, self._a_polyak,
                      self._a_advance):
                a.stream = s
            self._draw(s)
            api.check(self._sample(pol._h, n, mb.next_obs.data_ptr(), None, ids, self.seed, 0, self.action_range, r.a_next.data_ptr(),
                                   r.logp_next.data_ptr(), None, None, s))
            off.check(off.q_pack(C.byref(self._a_pack_next)))
            api.mlp_forward(self.targets[0]._handle, n, r.qin_next.data_ptr(), r.q1t.data_ptr(), s)
            api.mlp_forward(self.targets[1]._handle, n, r.qin_next.data_ptr(), r.q2t.data_ptr(), s)
            api.mlp_forward(q1._h, n, mb.qin.data_ptr(), r.q1.data_ptr(), s)
            api.mlp_forward(q2._h, n, mb.qin.data_ptr(), r.q2.data_ptr(), s)
            off.check(off.sac_critic(C.byref(self._a_critic)))
            self._after_critic(s)
            self._backward(q1, mb.qin, r.g_q1, None, self.adam_q1.grads[0], s)
            self._backward(q2, mb.qin, r.g_q2, None, self.adam_q2.grads[0], s)
            for adam, q in ((self.adam_q1, q1), (self.adam_q2, q2)):
                adam.issue()
                adam.bump()
                self._upload(q, s)
            api.check(self._sample(pol._h, n, mb.obs.data_ptr(), None, ids, self.seed, 1, self.action_range, r.a_new.data_ptr(),
                                   r.logp.data_ptr(), r.logits.data_ptr(), r.eps.data_ptr(), s))
            off.check(off.q_pack(C.byref(self._a_pack_new)))
            api.mlp_forward(q1._h, n, mb.qin.data_ptr(), r.q1n.data_ptr(), s)
            api.mlp_forward(q2._h, n, mb.qin.data_ptr(), r.q2n.data_ptr(), s)
            off.check(off.sac_actor(C.byref(self._a_actor)))
            self._backward(q1, mb.qin, r.ga_q1, r.g_in1, None, s)
            self._backward(q2, mb.qin, r.ga_q2, r.g_in2, None, s)
            off.check(off.q_action_grad(C.byref(self._a_grad)))
            api.check(self._vjp(n, 2 * self.buffer.act_dim, r.logits.data_ptr(), r.eps.data_ptr(), self.action_range, r.g_a.data_ptr(),
                                r.g_logp.data_ptr(), r.g_logits.data_ptr(), s))
            self._backward(pol, mb.obs, r.g_logits, None, self.adam_pi.grads[0], s)
            self.adam_pi.issue()
            self.adam_pi.bump()
            self._upload(pol, s)
            self.adam_alpha.issue()
            off.check(off.polyak(C.byref(self._a_polyak)))
            for t, flat in zip(self.targets, self.target_flat):
                api.mlp_set_params_device(t._handle, flat.data_ptr(), s)
            self._epoch.check(self._epoch.epoch_advance(C.byref(self._a_advance)))

    def capture(self, keep_graph=False):
        """a torch.cuda.CUDAGraph of one step(): a linear chain of KERNELS kernel nodes on one stream.  Nothing runs during the
        capture; every replay is one update on whatever the ring, the counter and the weights hold then.  Replay it with
        `self.replay(graph)` (train.PPOUpdate.capture explains why)."""
        import gc
        for net in (self.policy, self.q1, self.q2):
            net._sync()
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
        """graph.replay() and what step() does on the host after its launches: the versions of the three flat weight tensors move and
        `_uploaded` follows them.  No host read."""
        graph.replay()
        for adam in (self.adam_q1, self.adam_q2, self.adam_pi):
            adam.bump()
        for net in (self.policy, self.q1, self.q2):
            net._uploaded = net._flat._version

    def log(self):
        """the one device-to-host copy: the per-row outputs of the last update and log_alpha, folded on the host in float64 ->
        dict(critic1_loss, critic2_loss, actor_loss, alpha, logp, y)"""
        r = self.rows
        torch.stack([r.loss1, r.loss2, r.aloss, r.logp, r.y, self.log_alpha.expand(self.n), r.logp_next], out=self._log)
        host = self._log.cpu().numpy().astype(np.float64)
        return dict(critic1_loss=float(host[0].mean()), critic2_loss=float(host[1].mean()), actor_loss=float(host[2].mean()),
                    alpha=float(_exp_det(np.asarray([host[5][0]], _f))[0]), logp=float(host[3].mean()), y=float(host[4].mean()))
