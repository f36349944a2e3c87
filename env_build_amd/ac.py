"""A shared-trunk actor-critic for the PPO pipeline (include/envbuild_ac.h, env_build_amd/csrc/eb_ac.hip): ONE network with
W = 2 * act_dim + 1 outputs — the policy's mean and log-std in columns 0 .. 2A-1, as every other entry reads them, and the value in column
2A — instead of a policy and a value network over the same observations.  A minibatch is then one forward, one loss launch (eb_ac_loss:
the PPO row, the value-loss row and the WHOLE cotangent in ONE launch), one backward and Adam over one parameter set; during collection
the value of every visited state falls out of the forward that samples the action (eb_ac_sample, ONE launch).

This is an OPTION, not a replacement: a shared trunk is a different model from two networks, and nothing here claims it learns better.

`make_net(obs_dim, hidden_layers, units, hidden_activation, act_dim, ...)`: a `TrainableMLPNet` with 2 * act_dim + 1 linear outputs.
`split(net)` -> (policy `MLPNet` [2A outputs], value `MLPNet` [1 output]) with the trunk's weights and the matching output columns: how a
trained shared net reaches the consumers of a 2A-wide handle (Policy4Toyota, the shield, policy_rollout).  The output layer is one
ascending-k chain per column, so the split nets' outputs are the shared net's columns bit for bit.
`PPOUpdate(train.PPOUpdate)`: the minibatch chain, 8 kernels where the parent's is 13; `epoch.PPOEpochs` drives it unchanged.  With a
control (or lr_table / target_kl) the object made is a `ControlledPPOUpdate` — also a `ctl.PPOUpdate`, so `ctl.PPOEpochs` drives it unchanged.
`Collector(collect.Collector)`: the collection phase on the shared net; the same buffers, collect() / finish() / episodes() and dict.

`ac_loss_reference` and `ac_sample_reference` restate the header's contract by COMPOSITION of `ppo.ppo_reference`,
`train.value_loss_reference` and `policy_sample.policy_sample_reference` on strided views: no arithmetic is written a second time.

The entries live in env_build_amd/lib/libenvbuild_ac.so, a library of its own that is bound here on first use (AC_PROTOTYPES): the other
five libraries and _capi's tables stay as they are, and nothing but this module loads it.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from . import collect as _collect
from . import ctl as _ctl
from . import train as _train
from .dynamics_and_models import _stream

__all__ = ['make_net', 'split', 'PPOUpdate', 'ControlledPPOUpdate', 'Collector', 'ac_loss_reference', 'ac_sample_reference', 'EbAcLossArgs',
           'EbAcSampleArgs', 'EB_AC_ABI_VERSION', 'EB_AC_MAX_ACT_DIM', 'AC_PROTOTYPES', 'ac_api']

_P, _I, _F, _U64 = C.c_void_p, C.c_int32, C.c_float, C.c_uint64
EB_AC_ABI_VERSION = 1
EB_AC_MAX_ACT_DIM = 15
HEADER = 'envbuild_ac.h'


class EbAcLossArgs(C.Structure):
    """eb_ac_loss_args of include/envbuild_ac.h"""
    _fields_ = [('n', _I), ('act_dim', _I), ('y', _P), ('actions', _P), ('logp_old', _P), ('adv', _P), ('adv_norm', _P), ('ret', _P),
                ('v_old', _P), ('action_range', _F), ('clip', _F), ('ent_coef', _F), ('scale', _F), ('clip_v', _F), ('v_scale', _F),
                ('logp', _P), ('ratio', _P), ('surr', _P), ('ent', _P), ('vloss', _P), ('g_y', _P), ('z_out', _P), ('stream', _P)]


class EbAcSampleArgs(C.Structure):
    """eb_ac_sample_args"""
    _fields_ = [('n', _I), ('act_dim', _I), ('y', _P), ('eps', _P), ('row_ids', _P), ('seed', _U64), ('counter', _U64), ('action_range', _F),
                ('actions', _P), ('logits_out', _P), ('values', _P), ('logp', _P), ('eps_out', _P), ('stream', _P)]


# include/envbuild_ac.h: name -> (restype, argtypes) for every symbol the header declares
AC_PROTOTYPES = {
    'eb_ac_abi_version': (C.c_int, []),
    'eb_ac_last_error': (C.c_char_p, []),
    'eb_ac_loss': (C.c_int, [C.POINTER(EbAcLossArgs)]),
    'eb_ac_sample': (C.c_int, [C.POINTER(EbAcSampleArgs)]),
}


class AcApi(object):
    """libenvbuild_ac.so with its prototypes set; check(rc) raises with the library's own error string"""

    def __init__(self, path):
        if not os.path.isfile(path):
            raise _capi.EbError('shared library not found: %s' % path)
        self.path = path
        self.lib = C.CDLL(path)
        missing = [n for n in AC_PROTOTYPES if not hasattr(self.lib, n)]
        if missing:
            raise _capi.EbError('%s does not export %s (include/%s)' % (path, ', '.join(missing), HEADER))
        for n, (res, args) in AC_PROTOTYPES.items():
            fn = getattr(self.lib, n)
            fn.restype, fn.argtypes = res, args
        v = self.lib.eb_ac_abi_version()
        if v != EB_AC_ABI_VERSION:
            raise _capi.EbError('%s: ac ABI version %d, expected %d (include/%s)' % (path, v, EB_AC_ABI_VERSION, HEADER))
        self.loss, self.sample = self.lib.eb_ac_loss, self.lib.eb_ac_sample

    def check(self, rc):
        if rc != 0:
            msg = self.lib.eb_ac_last_error()
            msg = msg.decode() if msg else ''
            if rc == -1:
                raise ValueError('envbuild(ac): %s' % msg)
            raise _capi.EbError('envbuild(ac) error %d: %s' % (rc, msg))


_ac_api = None


def ac_api():
    """The actor-critic library, loaded on first use after the main one (one HIP runtime per process: PyTorch's).  Raises — never falls
    back — when it is absent or was built from other sources and cannot be rebuilt."""
    global _ac_api
    if _ac_api is None:
        _capi.hip_api()
        from . import build as _build
        if _build.ac_needs_build():
            hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
            if not os.path.isfile(hipcc):
                raise _capi.EbError('%s is missing or was built from other sources than the ones in %s — run `python -c "import '
                                    '__graft_entry__ as g; g.build()"` (hipcc --offload-arch=gfx950).  env_build_amd has no CPU fallback.'
                                    % (_build.AC_LIB, _build.CSRC))
            try:
                _build.build_ac()
            except Exception as e:   # noqa: BLE001
                raise _capi.EbError('building %s failed: %s.  env_build_amd has no CPU fallback.' % (_build.AC_LIB, e))
        _ac_api = AcApi(_build.AC_LIB)
    return _ac_api


def _ptr(t):
    return None if t is None else t.data_ptr()


def _act_dim(out_dim):
    """the act_dim of a shared net with out_dim = 2 * act_dim + 1 outputs"""
    out_dim = int(out_dim)
    if out_dim < 3 or out_dim % 2 == 0 or out_dim > 2 * EB_AC_MAX_ACT_DIM + 1:
        raise ValueError('a shared actor-critic network has 2 * act_dim + 1 outputs with act_dim in 1 .. %d, got %d outputs'
                         % (EB_AC_MAX_ACT_DIM, out_dim))
    return out_dim // 2


# ---- the network ---------------------------------------------------------------------------------------------------------------------------
def make_net(obs_dim, hidden_layers, units, hidden_activation, act_dim, **kwargs):
    """a `TrainableMLPNet` obs_dim -> 2 * act_dim + 1 with linear outputs: logits in columns 0 .. 2A-1, the value in column 2A.
    kwargs (name, device, seed) go to the network."""
    from .policy_grad import TrainableMLPNet
    A = int(act_dim)
    if not 1 <= A <= EB_AC_MAX_ACT_DIM:
        raise ValueError('act_dim must be in 1 .. %d, got %d' % (EB_AC_MAX_ACT_DIM, A))
    if kwargs.get('output_activation') not in (None, 'linear'):
        raise ValueError('the outputs of a shared actor-critic network are linear')
    kwargs = dict(kwargs, output_activation='linear')
    kwargs.setdefault('name', 'actor_critic')
    return TrainableMLPNet(int(obs_dim), int(hidden_layers), int(units), hidden_activation, 2 * A + 1, **kwargs)


def split(net):
    """(policy, value): two fp32 `MLPNet`s with the trunk's weights of the shared `net` as they are now and the output columns
    0 .. 2A-1 and 2A of its output layer; the observation scale goes with them.  Copies: a later step of `net` does not reach them."""
    from .policy import MLPNet
    if not isinstance(net, MLPNet):
        raise TypeError('split takes an MLPNet, got %s' % type(net).__name__)
    A = _act_dim(net.output_dim)
    w = net.get_weights()
    kernel, bias = w[-2], w[-1]
    out = []
    for name, cols in (('policy', slice(0, 2 * A)), ('value', slice(2 * A, 2 * A + 1))):
        part = MLPNet(net.input_dim, net.num_hidden_layers, net.num_hidden_units, net.hidden_activation, cols.stop - cols.start,
                      output_activation=net.output_activation, name='%s_%s' % (net.name, name), device=net.device)
        part.set_weights(w[:-2] + [np.ascontiguousarray(kernel[:, cols]), np.ascontiguousarray(bias[cols])])
        if net._obs_scale is not None:
            part.set_obs_scale(net._obs_scale)
        out.append(part)
    return tuple(out)


# ---- one PPO minibatch -------------------------------------------------------------------------------------------------------------------
class PPOUpdate(_train.PPOUpdate):
    """One PPO minibatch of `n_rows` rows for ONE shared `TrainableMLPNet` (`make_net`) as a fixed chain of 8 kernels on the current stream:

        eb_mlp_forward(net)             mb.obs -> y [n, 2A + 1]
        eb_ac_loss                      rows.logp, ratio, surr, ent, vloss; the whole cotangent g_y with scale = 1 / n_rows on the policy
                                        columns and vf_coef / n_rows on the value column
        eb_mlp_backward(net)            head = 0, into the net's flat gradient                            (3 kernels)
        eb_adam_step                    over the one net                                                  (2 kernels)
        eb_mlp_set_params_device        the inference handle current again

    The parent's chain is 13: two forwards, two backwards, two uploads.  `mb.*`, `rows.*`, `adam`, `n`, `device`, `_ppo_args.clip`,
    capture() and replay() are the parent's; `policy` and `value` both name the one net, so `epoch.PPOEpochs` drives this object
    unchanged.  With `control` (a `ctl.UpdateControl`), `lr_table` or `target_kl` the object made is a `ControlledPPOUpdate`: its optimiser
    is `ctl.Adam` — 8 kernels, 10 with target_kl — and `ctl.PPOEpochs` drives it unchanged.
    step() makes no torch operation, no host read, no allocation and no autograd."""

    def __new__(cls, *args, **kw):
        if cls is PPOUpdate and any(kw.get(k) is not None for k in ('control', 'lr_table', 'target_kl')):
            cls = ControlledPPOUpdate
        return object.__new__(cls)

    def __init__(self, net, n_rows, action_range, clip, ent_coef=0.0, vf_coef=0.5, clip_v=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=None, control=None, lr_table=None, target_kl=None, kl_factor=1.5, max_slots=1024):
        from .policy_grad import TrainableMLPNet
        from .policy_sample import _range
        if not isinstance(net, TrainableMLPNet):
            raise TypeError('PPOUpdate trains a TrainableMLPNet, got %s' % type(net).__name__)
        A = _act_dim(net.output_dim)
        if net.precision != 'fp32':
            raise ValueError('the shared network %s must be fp32, got %r: an fp16 handle has no gradient' % (net.name, net.precision))
        n = int(n_rows)
        if n < 1:
            raise ValueError('n_rows must be at least 1')
        if control is None and (lr_table is not None or target_kl is not None or isinstance(self, _ctl.PPOUpdate)):
            control = _ctl.UpdateControl(net.device, lr_table=lr_table, target_kl=target_kl, kl_factor=kl_factor, max_slots=max_slots)
        elif control is not None and (lr_table is not None or target_kl is not None):
            raise ValueError('pass a control, or lr_table / target_kl to make one, not both')
        self.control = control
        self.policy = self.value = self.net = net
        self.n, self.device, self.api, self.act_dim = n, net.device, net.api, A
        dev, f32, W = self.device, torch.float32, net.output_dim
        new = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        self.mb = _train._Buffers(obs=new(n, net.input_dim), actions=new(n, A), logp_old=new(n), adv=new(n), ret=new(n), v_old=new(n),
                                  adv_norm=torch.tensor([0.0, 1.0], dtype=f32, device=dev))
        self.rows = _train._Buffers(logp=new(n), ratio=new(n), surr=new(n), ent=new(n), vloss=new(n))
        self.y, self.g_y = new(n, W), new(n, W)
        self.adam = self._make_adam([net], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        net._sync()                                              # a handle that has never been uploaded has no layers yet
        need = C.c_size_t(0)
        self.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
        self._ws = [(torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev), need.value)]
        ent_coef = float(np.float32(_train._scalar(ent_coef, 'ent_coef')))
        self.vf_coef = _train._scalar(vf_coef, 'vf_coef')
        self._ac = ac_api()
        self._ppo_args = EbAcLossArgs(n=n, act_dim=A, y=_ptr(self.y), actions=_ptr(self.mb.actions), logp_old=_ptr(self.mb.logp_old),
                                      adv=_ptr(self.mb.adv), adv_norm=_ptr(self.mb.adv_norm), ret=_ptr(self.mb.ret),
                                      v_old=None if clip_v is None else _ptr(self.mb.v_old), action_range=_range(action_range),
                                      clip=_train._scalar(clip, 'clip', 0.0), ent_coef=ent_coef, scale=1.0 / n,
                                      clip_v=0.0 if clip_v is None else _train._scalar(clip_v, 'clip_v', 0.0), v_scale=self.vf_coef / n,
                                      logp=_ptr(self.rows.logp), ratio=_ptr(self.rows.ratio), surr=_ptr(self.rows.surr),
                                      ent=_ptr(self.rows.ent), vloss=_ptr(self.rows.vloss), g_y=_ptr(self.g_y))

    def _make_adam(self, nets, **kw):
        """train.Adam, or — under a control — ctl.Adam watching rows.logp and mb.logp_old when the control has a target_kl"""
        if self.control is None:
            return _train.Adam(nets, **kw)
        adam = _ctl.Adam(nets, self.control, **kw)
        if self.control.limit is not None:
            adam.watch(self.rows.logp, self.mb.logp_old)
        return adam

    def step(self):
        """the chain, on the current stream"""
        net, api, n = self.net, self.api, self.n
        net._sync()
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            obs = self.mb.obs.data_ptr()
            api.mlp_forward(net._h, n, obs, self.y.data_ptr(), s)
            self._ppo_args.stream = s
            self._ac.check(self._ac.loss(C.byref(self._ppo_args)))
            (ws, need), g = self._ws[0], self.adam.grads[0]
            api.mlp_backward(net._h, n, obs, self.g_y.data_ptr(), 0, 0.0, ws.data_ptr(), need, None, None, g.data_ptr(), s)
            self.adam.issue()
            self.adam.bump()
            api.mlp_set_params_device(net._h, net._flat.data_ptr(), s)
            net._uploaded = net._flat._version


class ControlledPPOUpdate(PPOUpdate, _ctl.PPOUpdate):
    """`PPOUpdate` under a `ctl.UpdateControl`: the same object and the same chain — it only is a `ctl.PPOUpdate` too, which is what
    `ctl.PPOEpochs` asks of its update.  `PPOUpdate(..., control= / lr_table= / target_kl=)` makes one."""


# ---- the collector --------------------------------------------------------------------------------------------------------------------------
class Collector(_collect.Collector):
    """`collect.Collector` on ONE shared net: the same buffers, collect() / finish() / episodes() and returned dict, everything a library
    launch on the current stream:

        collect():   eb_collect_begin(env's observation -> obs_buf[0])                                          (1 kernel)
                     for t in 0 .. T - 1:
                         eb_mlp_forward(obs_buf[t] -> y_buf[t])                                                  (1 kernel)
                         eb_ac_sample(y_buf[t] -> act_buf[t], logit_buf[t], values[t]; counter = iteration * T + t)   (1 kernel)
                         env.step(act_buf[t])                                                                   (eb_env_step)
                         eb_collect_record(t)                                                                   (1 kernel)
        finish(gamma, lam):
                     eb_mlp_forward(obs_buf[T] -> y_last), eb_ac_sample(split only -> values[T])                 B rows
                     eb_mlp_forward(trunc_obs -> y_trunc), eb_ac_sample(split only -> v_trunc)                   B rows
                     eb_collect_next_values
                     eb_policy_logp_from_logits(logit_buf, act_buf -> logp_old)
                     eb_gae(rew_buf, values, nonterminal, next_values, carry -> adv, ret)

    The value of every visited state falls out of the forward that samples its action: there is no forward over (T + 1) * B rows.
    logit_buf is dense [T, B, 2A], so eb_policy_logp_from_logits and the rest of the head are the parent's, unchanged.  `net`: an fp32
    MLPNet / TrainableMLPNet with 2 * act_dim + 1 outputs (`make_net`).  `policy` and `value` both name it."""

    def __init__(self, env, net, steps, action_range, seed=0):
        from . import policy_logp, policy_sample, ppo
        from .endtoend import CrossroadEnd2end
        from .policy import MLPNet
        if not isinstance(env, CrossroadEnd2end):
            raise TypeError('Collector drives a CrossroadEnd2end, got %s' % type(env).__name__)
        if not env.auto_reset or env.copy_outputs or env.n_env < 2:
            raise ValueError('Collector needs an env with auto_reset=True, copy_outputs=False and n_env > 1')
        if not isinstance(net, MLPNet):
            raise TypeError('net must be an MLPNet')
        T, B, D = int(steps), env.n_env, env.obs_dim
        if T < 1 or T > 65535:
            raise ValueError('steps must be in 1 .. 65535 (eb_gae), got %d' % T)
        if env.max_episode_steps is not None and T > env.max_episode_steps:
            raise ValueError('steps = %d exceeds env.max_episode_steps = %d: an env could be truncated twice within one collection, and the '
                             'buffer keeps one final observation per env' % (T, env.max_episode_steps))
        dev = env.device
        if net.device != dev:
            raise ValueError('the network must live on the device of the env')
        A = _act_dim(net.output_dim)
        if net.input_dim != D or A != env.action_number:
            raise ValueError('the shared network must map %d -> 2 * %d + 1, got %d -> %d' % (D, env.action_number, net.input_dim, net.output_dim))
        if net.precision != 'fp32':
            raise ValueError('Collector: the shared network %s must be fp32, got %r' % (net.name, net.precision))
        self.env, self.net = env, net
        self.policy = self.value = net
        self.steps, self.n_env, self.obs_dim, self.act_dim, self.device = T, B, D, A, dev
        self.action_range, self.seed, self.iteration = policy_sample._range(action_range), int(seed) & ((1 << 64) - 1), 0
        f32, W = dict(dtype=torch.float32, device=dev), net.output_dim
        self.buf = _collect.buffers(T, B, D, dev)
        self.act_buf, self.logit_buf = torch.zeros((T, B, A), **f32), torch.zeros((T, B, 2 * A), **f32)
        self.y_buf, self.y_last, self.y_trunc = torch.zeros((T, B, W), **f32), torch.zeros((B, W), **f32), torch.zeros((B, W), **f32)
        self.values, self.v_trunc = torch.zeros((T + 1, B), **f32), torch.zeros((B,), **f32)
        self.next_values, self.logp_old = torch.zeros((T, B), **f32), torch.zeros((T * B,), **f32)
        self.adv, self.ret = torch.zeros((T, B), **f32), torch.zeros((T, B), **f32)
        self.log_blocks = torch.zeros((_collect.EB_COLLECT_LOG_BLOCKS, _collect.EB_COLLECT_LOG_FIELDS), dtype=torch.float64, device=dev)
        self.api, self._ac = _collect.collect_api(), ac_api()
        self._logp_fn = policy_logp.bind(net.api)['eb_policy_logp_from_logits']
        self._gae_fn = ppo.bind(net.api)['eb_gae']
        obs_buf = self.buf['obs_buf']
        self._obs_at = [obs_buf[t].data_ptr() for t in range(T + 1)]
        self._act_at = [self.act_buf[t] for t in range(T)]                  # what env.step takes: views made once
        self._y_at = [self.y_buf[t].data_ptr() for t in range(T)]
        self._samples = [EbAcSampleArgs(n=B, act_dim=A, y=self._y_at[t], seed=self.seed, action_range=self.action_range,
                                        actions=_ptr(self.act_buf[t]), logits_out=_ptr(self.logit_buf[t]), values=_ptr(self.values[t]))
                         for t in range(T)]
        self._split_last = EbAcSampleArgs(n=B, act_dim=A, y=_ptr(self.y_last), action_range=self.action_range, values=_ptr(self.values[T]))
        self._split_trunc = EbAcSampleArgs(n=B, act_dim=A, y=_ptr(self.y_trunc), action_range=self.action_range, values=_ptr(self.v_trunc))
        self._begin = _collect.EbCollectBeginArgs(n_env=B, obs_dim=D, obs_buf=_ptr(obs_buf), trunc_t=_ptr(self.buf['trunc_t']))
        self._records = [_collect._record_args(t, self.buf) for t in range(T)]
        self._next = _collect._next_values_args(self.values, self.v_trunc, self.buf['trunc_t'], self.next_values)
        self._logp = policy_logp._args(None, T * B, 2 * A, self.action_range, logits=self.logit_buf, actions=self.act_buf, logp=self.logp_old)
        self._gae = ppo._gae_args(None, T, B, 0.0, 0.0, rewards=self.buf['rew_buf'], values=self.values, nonterminal=self.buf['nonterminal'],
                                  next_values=self.next_values, carry=self.buf['carry'], adv=self.adv, ret=self.ret)
        self._log = _collect._episode_log_args(self.buf['ret_buf'], self.buf['len_buf'], self.buf['code_buf'], self.log_blocks)
        self.data = dict(obs=obs_buf[:T].view(T * B, D), actions=self.act_buf.view(T * B, A), logp_old=self.logp_old, adv=self.adv.view(T * B),
                         ret=self.ret.view(T * B), v_old=self.values[:T].view(T * B))

    def collect(self):
        """T steps from the env's current observation into the buffer; the env is left T steps further"""
        api, ac, env, net, T, B = self.api, self._ac, self.env, self.net, self.steps, self.n_env
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            h = net._handle                                       # (a TrainableMLPNet uploads weights written since the last launch)
            a = self._begin
            a.obs, a.stream = env.obs.t.data_ptr(), s
            api.check(api.begin(C.byref(a)))
            base = self.iteration * T
            for t in range(T):
                net.api.mlp_forward(h, B, self._obs_at[t], self._y_at[t], s)
                sm = self._samples[t]
                sm.counter, sm.stream = base + t, s
                ac.check(ac.sample(C.byref(sm)))
                obs, reward, _done, info = env.step(self._act_at[t])
                r = self._records[t]
                _collect._set_step(r, obs.t, reward.t, env.done_code, info['final_observation'].t)
                r.stream = s
                api.check(api.record(C.byref(r)))
        self.iteration += 1

    def finish(self, gamma, lam):
        """the head of the update on what collect() left -> the dict epoch.PPOEpochs takes (views of this object's buffers)"""
        api, ac, net, T, B = self.api, self._ac, self.net, self.steps, self.n_env
        g, l = float(gamma), float(lam)
        if not (np.isfinite(g) and np.isfinite(l)):
            raise ValueError('gamma and lam must be finite, got %r and %r' % (gamma, lam))
        with torch.cuda.device(self.device):
            s = _stream(self.device)
            h = net._handle
            for obs, y, sp in ((self._obs_at[T], self.y_last, self._split_last), (self.buf['trunc_obs'].data_ptr(), self.y_trunc, self._split_trunc)):
                net.api.mlp_forward(h, B, obs, y.data_ptr(), s)
                sp.stream = s
                ac.check(ac.sample(C.byref(sp)))
            self._next.stream = s
            api.check(api.next_values(C.byref(self._next)))
            self._logp.stream = s
            net.api.check(self._logp_fn(C.byref(self._logp)))
            self._gae.gamma, self._gae.lam, self._gae.stream = g, l, s
            net.api.check(self._gae_fn(C.byref(self._gae)))
        return self.data


# ---- the contract in NumPy, by composition ---------------------------------------------------------------------------------------------
def ac_loss_reference(y, actions, logp_old, adv, ret, action_range, clip, ent_coef=0.0, scale=None, adv_norm=None, v_old=None, clip_v=0.0,
                      v_scale=None, dtype=np.float32):
    """eb_ac_loss in NumPy on y [n, 2A + 1] -> dict(logp, z, A, ratio, surr, ent, g_lp, vloss, g_y [n, 2A + 1]): `ppo.ppo_reference` on
    the view y[:, :2A] and `train.value_loss_reference` on the view y[:, 2A], nothing else.  scale and v_scale None: 1 / n."""
    from .ppo import ppo_reference
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError('y must be [n, 2 * act_dim + 1], got %s' % (y.shape,))
    A = _act_dim(y.shape[1])
    out = ppo_reference(y[:, :2 * A], actions, logp_old, adv, action_range, clip, ent_coef=ent_coef, scale=scale, adv_norm=adv_norm, dtype=dtype)
    vloss, g_v = _train.value_loss_reference(y[:, 2 * A], ret, v_old=v_old, clip_v=clip_v, scale=v_scale, dtype=dtype)
    g_y = np.concatenate([out.pop('g_logits'), g_v.reshape(-1, 1)], axis=1)
    out.pop('loss')
    out.update(vloss=vloss, g_y=g_y)
    return out


def ac_sample_reference(y, eps, action_range, dtype=np.float32):
    """eb_ac_sample in NumPy on y [n, 2A + 1] and the noise eps [n, A] (`policy_sample.policy_noise_reference` gives the kernel's) ->
    dict(actions, logp, logits [n, 2A], values [n]): `policy_sample.policy_sample_reference` on the view y[:, :2A], and two copies."""
    from .policy_sample import policy_sample_reference
    y = np.asarray(y)
    if y.ndim != 2:
        raise ValueError('y must be [n, 2 * act_dim + 1], got %s' % (y.shape,))
    A = _act_dim(y.shape[1])
    actions, logp, _ = policy_sample_reference(y[:, :2 * A], eps, action_range, dtype=dtype)
    return dict(actions=actions, logp=logp, logits=np.ascontiguousarray(y[:, :2 * A], np.float32), values=np.ascontiguousarray(y[:, 2 * A], np.float32))
