"""The policy side of the reference's decision loop, on the GPU: `MLPNet` (utils/model.py:18-43), `Policy4Toyota`
(utils/policy.py:19-101, the inference surface, deterministic and stochastic) and `LoadPolicy` (utils/load_policy.py:19-63) with
the 'scale' observation preprocessor (utils/preprocessor.py:116-123).

Same names, constructor arguments and methods as the reference; the arithmetic is one fused HIP kernel per call
(env_build_amd/csrc/eb_policy.hip: fp32 matrix cores, the whole network in one launch; with precision='fp16' the opt-in
binary16 kernel of env_build_amd/csrc/eb_policy_f16.hip, include/envbuild_mlp_f16.h).  The shield and the path selection
only ever call `run_batch` / `obj_value_batch`; the network's backward and a trainable `MLPNet` whose weights stay on the
device are env_build_amd.policy_grad (`TrainableMLPNet`, include/envbuild_mlp_grad.h).  With deterministic_policy false,
`compute_action` samples the tanh-Gaussian policy and returns the actions with their log-probabilities in one launch
(env_build_amd.policy_sample, include/envbuild_policy_sample.h); `seed` makes the draws repeat.  Optimisers are out of scope.

TensorFlow checkpoints cannot be read here (no TF, and the reference's checkpoints are git-ignored): weights are
exchanged as the list `Model.get_weights()` returns — [kernel0, bias0, kernel1, bias1, ...], kernels [in, out] —
or as an .npz of that list (`save_weights` / `load_weights`).  There is no CPU path.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _capi
from .dynamics_and_models import DevArray, _dev, _resolve_device, _stream

__all__ = ['MLPNet', 'Policy4Toyota', 'LoadPolicy', 'orthogonal', 'mlp_f16_reference']


def orthogonal(rng, rows, cols, gain):
    """tf.keras.initializers.Orthogonal(gain) for a [rows, cols] kernel: QR of a normal matrix, sign-fixed."""
    a = rng.standard_normal((max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    if rows < cols:
        q = q.T
    return (gain * q[:rows, :cols]).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays through float64: the product is exact there, the sum rounds twice (float64, then float32)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _exp_det(x0, fma=_fma32):
    """csrc/eb_mlp_device.h:exp_det (the oracle's eb_expf) on a float32 array; `fma`: the fused multiply-add it is evaluated with."""
    x0 = np.asarray(x0, np.float32)
    with np.errstate(all='ignore'):
        x = np.where(x0 > 88, np.float32(88), np.where(x0 < -87, np.float32(-87), x0)).astype(np.float32)
        fx = np.rint(x * np.float32(1.44269504088896341)).astype(np.float32)
        r = fma(-fx, np.float32(0.693359375), x)
        r = fma(-fx, np.float32(-2.12194440e-4), r)
        z = r * r
        p = np.full_like(r, 1.9875691500e-4)
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = fma(p, r, np.float32(c))
        y = fma(p, z, r) + np.float32(1)
        n = np.where(np.isnan(x0), 0, fx).astype(np.int32)
        v = y * ((n + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
    return np.where(np.isnan(x0), x0, v).astype(np.float32)


def _tanh_det(x, fma=_fma32):
    """csrc/eb_mlp_device.h:tanh_det (the oracle's eb_tanhf) on a float32 array; `fma` as in _exp_det."""
    x = np.asarray(x, np.float32)
    with np.errstate(all='ignore'):
        ax = np.abs(x)
        s = _exp_det(ax + ax, fma)
        t = np.float32(1) - np.float32(2) / (s + np.float32(1))
        big = np.where(x < 0, -t, t)
        z = x * x
        p = np.full_like(x, -5.70498872745e-3)
        for c in (2.06390887954e-2, -5.37397155531e-2, 1.33314422036e-1, -3.33332819422e-1):
            p = fma(p, z, np.float32(c))
        small = fma(p * z, x, x)
        sat = np.where(x > 0, np.float32(1), np.float32(-1))
    return np.where(ax > 44, sat, np.where(ax >= 0.625, big, small)).astype(np.float32)


def _act_det(act, x):
    x = np.asarray(x, np.float32)
    if act == 'relu':
        return np.where(x > 0, x, np.float32(0)).astype(np.float32)
    if act == 'elu':
        with np.errstate(all='ignore'):
            return np.where(x > 0, x, _exp_det(x) - np.float32(1)).astype(np.float32)
    if act == 'tanh':
        return _tanh_det(x)
    return x


def mlp_f16_reference(layers, obs, hidden_act, out_act, obs_scale=None, accumulate=np.float32, k_block=None, reverse=False):
    """The arithmetic contract of include/envbuild_mlp_f16.h in NumPy — the counterpart of `sample.sample_tapes_reference`: what
    eb_mlp_forward gives on a handle whose precision is 'fp16', up to the order of each sum.

    layers: [(kernel [in, out], bias [out]), ...]; obs [n, in] float32.  Inputs, weights and hidden activations are rounded with
    astype(np.float16) (IEEE round-to-nearest-even, overflow to inf, subnormals kept: so does the kernel); biases stay float32;
    a pre-activation is the bias plus the products (exact in float32) summed in `accumulate` (np.float32 or np.float64) in ascending
    k; the activation is the deterministic float32 one (its fused multiply-adds go through float64 here: a last-bit difference from
    fmaf is possible where that rounds twice), and the output layer's result is float32.

    k_block / reverse give a second accumulation order for tests: the products of each block of k_block consecutive k are summed
    exactly (float64), rounded once to `accumulate`, and the blocks are added in ascending (or, with reverse, descending) order.
    The kernel's own order is neither: the contract leaves it open."""
    acc_t = np.dtype(accumulate).type
    x = np.asarray(obs, np.float32)
    if obs_scale is not None:
        x = x * np.asarray(obs_scale, np.float32)
    with np.errstate(all='ignore'):
        x = x.astype(np.float16)
        for L, (w, b) in enumerate(layers):
            w16 = np.asarray(w, np.float32).astype(np.float16)
            K = w16.shape[0]
            acc = np.broadcast_to(np.asarray(b, np.float32).astype(acc_t), (x.shape[0], w16.shape[1])).copy()
            if k_block is None:
                for k in range(K):       # float32 products of binary16 values are exact
                    acc = acc + (x[:, k:k + 1].astype(np.float32) * w16[k:k + 1, :].astype(np.float32)).astype(acc_t)
            else:
                starts = list(range(0, K, k_block))
                for k0 in (reversed(starts) if reverse else starts):
                    part = x[:, k0:k0 + k_block].astype(np.float64) @ w16[k0:k0 + k_block, :].astype(np.float64)
                    acc = acc + part.astype(acc_t)
            pre = acc.astype(np.float32)
            if L == len(layers) - 1:
                return _act_det(out_act, pre)
            x = _act_det(hidden_act, pre).astype(np.float16)


class MLPNet(object):
    """utils/model.py:18-43.  `hidden_activation` / `output_activation` in {'elu', 'relu', 'tanh', 'linear', None}.
    `precision` in {'fp32', 'fp16'}: 'fp32' (the default) is the bit-exact fp32 chain; 'fp16' evaluates with binary16 operands on the
    matrix cores (include/envbuild_mlp_f16.h) — faster, not reproducible bit for bit on the CPU."""

    def __init__(self, input_dim, num_hidden_layers, num_hidden_units, hidden_activation, output_dim, **kwargs):
        self.name = kwargs.get('name', 'mlp')
        self.input_dim, self.num_hidden_layers = int(input_dim), int(num_hidden_layers)
        self.num_hidden_units, self.output_dim = int(num_hidden_units), int(output_dim)
        self.hidden_activation = hidden_activation
        self.output_activation = kwargs.get('output_activation') or 'linear'
        for a in (self.hidden_activation, self.output_activation):
            if a not in _capi.ACT_ID:
                raise ValueError('unsupported activation %r' % (a,))
        dev = kwargs.get('device')
        self.device = _resolve_device(dev)
        self.api = _capi.hip_api()
        self._obs_scale = None
        self._handle = None
        self.precision = kwargs.get('precision', 'fp32')
        self._check_precision(self.precision)
        rng = np.random.default_rng(kwargs.get('seed', 0))
        dims = [self.input_dim] + [self.num_hidden_units] * self.num_hidden_layers + [self.output_dim]
        w = []
        for L in range(self.num_hidden_layers + 1):      # Orthogonal(sqrt 2) hidden, Orthogonal(1) output, zero bias
            gain = np.sqrt(2.) if L < self.num_hidden_layers else 1.
            w += [orthogonal(rng, dims[L], dims[L + 1], gain), np.zeros((dims[L + 1],), np.float32)]
        self.set_weights(w)

    # -- weights ------------------------------------------------------------------------------
    def get_weights(self):
        return [a.copy() for a in self._weights]

    def set_weights(self, weights):
        weights = [np.ascontiguousarray(a, np.float32) for a in weights]
        if len(weights) != 2 * (self.num_hidden_layers + 1):
            raise ValueError('expected %d arrays (kernel, bias per Dense layer)' % (2 * (self.num_hidden_layers + 1)))
        self._weights = weights
        self._rebuild()

    def set_obs_scale(self, obs_scale):
        """Preprocessor 'scale' (utils/preprocessor.py:121): applied inside the kernel while staging the input."""
        self._obs_scale = None if obs_scale is None else np.ascontiguousarray(obs_scale, np.float32)
        self._rebuild()

    @staticmethod
    def _check_precision(precision):
        if precision not in _capi.MLP_PRECISION_ID:
            raise ValueError("precision must be 'fp32' or 'fp16', got %r" % (precision,))

    def set_precision(self, precision):
        """'fp32' | 'fp16': what every later forward, `mode` and the native shield evaluate this network with.  The weights are kept
        in both packings, so the switch is a flag."""
        self._check_precision(precision)
        self.api.mlp_set_precision(self._handle, _capi.MLP_PRECISION_ID[precision])
        self.precision = precision

    def _rebuild(self):
        layers = list(zip(self._weights[0::2], self._weights[1::2]))
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        new = self.api.mlp_create_from(self.input_dim, self.num_hidden_layers, self.num_hidden_units, self.output_dim,
                                       self.hidden_activation, self.output_activation, layers, self._obs_scale, index)
        if self.precision != 'fp32':
            try:
                self.api.mlp_set_precision(new, _capi.MLP_PRECISION_ID[self.precision])
            except Exception:
                self.api.lib.eb_mlp_destroy(new)
                raise
        if self._handle is not None:
            torch.cuda.synchronize(self.device)
            self.api.lib.eb_mlp_destroy(self._handle)
        self._handle = new

    def __del__(self):
        try:
            if self._handle is not None:
                self.api.lib.eb_mlp_destroy(self._handle)
        except Exception:
            pass

    # -- forward ------------------------------------------------------------------------------
    def _in(self, x):
        t = _dev(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.input_dim:
            raise ValueError('input must be [B, %d], got %s' % (self.input_dim, tuple(t.shape)))
        return t

    def _stream(self):
        return _stream(self.device)

    def call(self, x, **kwargs):                       # utils/model.py:39-43
        t = self._in(x)
        out = torch.empty((t.shape[0], self.output_dim), dtype=torch.float32, device=self.device)
        self.api.mlp_forward(self._handle, t.shape[0], C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), self._stream())
        return DevArray(out)

    __call__ = call

    def mode(self, x, action_range):
        """action_range * tanh(mean) (utils/policy.py:68-72, 89-92) without materialising the logits."""
        t = self._in(x)
        out = torch.empty((t.shape[0], self.output_dim // 2), dtype=torch.float32, device=self.device)
        self.api.policy_run_batch(self._handle, t.shape[0], C.c_void_p(t.data_ptr()),
                                  C.c_float(-1.0 if action_range is None else float(action_range)),
                                  C.c_void_p(out.data_ptr()), self._stream())
        return DevArray(out)


class Policy4Toyota(object):
    """utils/policy.py:19-101, inference side.  `args` carries obs_dim, act_dim, num_hidden_layers, num_hidden_units,
    hidden_activation, policy_out_activation, action_range, deterministic_policy (as the experiment's config.json), and optionally
    policy_precision ('fp32', the default, or 'fp16': MLPNet's `precision`, for both networks)."""

    def __init__(self, args, device=None, seed=0):
        self.args = args
        obs_dim, act_dim = int(args.obs_dim), int(args.act_dim)
        n_hiddens, n_units, act = int(args.num_hidden_layers), int(args.num_hidden_units), args.hidden_activation
        precision = getattr(args, 'policy_precision', 'fp32') or 'fp32'
        self.policy = MLPNet(obs_dim, n_hiddens, n_units, act, act_dim * 2, name='policy',
                             output_activation=getattr(args, 'policy_out_activation', 'linear'), device=device, seed=seed,
                             precision=precision)
        self.obj_v = MLPNet(obs_dim, n_hiddens, n_units, act, 1, name='obj_v', output_activation='relu',
                            device=device, seed=seed + 1, precision=precision)
        self.models = (self.obj_v, self.policy,)
        self._sample_seed, self._sample_counter = int(seed), 0

    def seed(self, seed):
        """Restart the stochastic branch's noise stream: call k after seed(s) draws from (s, k), whatever came before."""
        self._sample_seed, self._sample_counter = int(seed), 0

    def get_weights(self):
        return [model.get_weights() for model in self.models]

    def set_weights(self, weights):
        for i, weight in enumerate(weights):
            self.models[i].set_weights(weight)

    def save_weights(self, save_dir, iteration):
        os.makedirs(save_dir, exist_ok=True)
        arrays = {'%s_%d' % (m.name, k): a for m in self.models for k, a in enumerate(m.get_weights())}
        np.savez(os.path.join(save_dir, 'weights_ite%d.npz' % int(iteration)), **arrays)

    def load_weights(self, load_dir, iteration):
        z = np.load(os.path.join(load_dir, 'weights_ite%d.npz' % int(iteration)))
        for m in self.models:
            m.set_weights([z['%s_%d' % (m.name, k)] for k in range(2 * (m.num_hidden_layers + 1))])

    def compute_mode(self, obs):                       # utils/policy.py:68-72
        return self.policy.mode(obs, getattr(self.args, 'action_range', None))

    def compute_action(self, obs):                     # utils/policy.py:85-98
        if not getattr(self.args, 'deterministic_policy', True):
            from .policy_sample import sample_actions
            out = sample_actions(self.policy, obs, getattr(self.args, 'action_range', None), seed=self._sample_seed,
                                 counter=self._sample_counter)
            self._sample_counter += 1
            return out['actions'], out['logp']
        return self.compute_mode(obs), 0.

    def compute_logp(self, obs, actions):              # utils/policy.py:71-82: _logits2dist(logits).log_prob(actions)
        from .policy_logp import log_prob_actions
        return log_prob_actions(self.policy, obs, actions, getattr(self.args, 'action_range', None))['logp']

    def compute_obj_v(self, obs):                      # utils/policy.py:100-103
        return DevArray(self.obj_v(obs).t[:, 0])


class LoadPolicy(object):
    """utils/load_policy.py:19-63.  `exp_dir/config.json` holds the arguments; the weights come from
    `exp_dir/models/weights_ite{iter}.npz` when present (else the random initialisation stands — useful for
    benchmarks).  The 'scale' preprocessor is folded into the kernels and the 'normalize' one (env_build_amd.norm.Preprocessor, its
    parameters from `exp_dir/models/ppc_params.npz` or the reference's `ppc_params.npy` when present) runs as one launch in front of them,
    so run_batch / obj_value_batch take raw obs."""

    def __init__(self, exp_dir=None, iter=None, args=None, device=None):
        if args is None:
            params = json.loads(open(os.path.join(exp_dir, 'config.json')).read())
            args = SimpleNamespace(**params)
        elif isinstance(args, dict):
            args = SimpleNamespace(**args)
        self.args = args
        self.policy = Policy4Toyota(args, device=device)
        self.preprocessor, self._scratch = None, None
        if exp_dir is not None and iter is not None:
            self.policy.load_weights(os.path.join(exp_dir, 'models'), iter)
        if getattr(args, 'obs_preprocess_type', 'scale') == 'scale' and getattr(args, 'obs_scale', None) is not None:
            scale = np.asarray(args.obs_scale, np.float32)
            for m in self.policy.models:
                m.set_obs_scale(scale)
        elif getattr(args, 'obs_preprocess_type', None) == 'normalize':
            from .norm import Preprocessor             # utils/load_policy.py:32-34: running statistics, on the device (envbuild_norm.h)
            self.preprocessor = Preprocessor((int(args.obs_dim),), 'normalize', getattr(args, 'reward_preprocess_type', None),
                                             gamma=getattr(args, 'gamma', 0.99), device=self.policy.policy.device)
            models = os.path.join(exp_dir, 'models') if exp_dir is not None else None
            if models is not None and any(os.path.isfile(os.path.join(models, 'ppc_params' + e)) for e in ('.npz', '.npy')):
                self.preprocessor.load_params(models)

    def _processed(self, obses):
        """eb_norm_apply into a scratch tensor in front of the network when the preprocessor is 'normalize'; else obses as they are"""
        if self.preprocessor is None:
            return obses
        from .norm import apply
        x = _dev(obses, self.policy.policy.device)
        if self._scratch is None or self._scratch.shape != x.shape:
            self._scratch = torch.empty_like(x)
        apply(self.preprocessor.ob_rms, x, self._scratch, self.preprocessor.clipob)
        return self._scratch

    def run_batch(self, obses):                        # utils/load_policy.py:53-57
        actions, _ = self.policy.compute_action(self._processed(obses))
        return actions

    def obj_value_batch(self, obses):                  # utils/load_policy.py:59-63
        return self.policy.compute_obj_v(self._processed(obses))

    __call__ = run_batch
