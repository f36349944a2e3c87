"""Shared by tests/test_policy_rollout_grad_fixture_host.py and tests/test_gpu_policy_rollout_fixture.py: the closed-loop gradient
fixtures G21 (scripts/gen_golden_policy_grad.py: the reference's model in closed loop with a torch MLP, differentiated by torch.autograd
in float64 and float32) and the bar they carry, which is tests/_grad_cases.py's:

    |g - g_float64_ref| <= 4 * E + 2**-20 * max |g_float64_ref|,   E = max |g_float32_ref - g_float64_ref|

per column of the row-wise outputs (g_obs0 [n, 9]; g_actions_steps [steps, n, 2], every step of a row held to its column's bound) and
per parameter tensor.  Every stored row meets the generator's conditions (`ok` is all true): g_params is a sum over rows, so no row
can be left out.  A helper module: pytest does not collect it, and importing it touches no device."""
import json

import numpy as np

from tests._grad_cases import TASKS, check_columns, column_tolerance
from tests._helpers import golden

MAX_BYTES = 591861            # tests/test_grad_host.py's bound: the largest fixture before the gradient ones
RTOL, ATOL = 1e-5, 5e-6       # the forward of a reference-generated fixture (tests/test_gpu_parity.py)


def stem(task):
    return 'g21_policy_rollout_grad_%s' % task


class Case(object):
    def __init__(self, z, task, name, meta):
        self.task, self.name, self.meta, self._z = task, name, meta, z
        self.entry, self.mode, self.n_veh, self.steps = meta['entry'], meta['mode'], meta['n_veh'], meta['steps']
        self.ar, self.sampled, self.hact = meta['action_range'], meta['sampled'], meta['hidden_activation']
        self.obs0, self.n = z[meta['rows'] + '/obs0'], len(z[meta['rows'] + '/obs0'])
        self.D = self.obs0.shape[1]
        self.dims = (self.D, meta['n_hidden'], meta['units'], 4)
        self.weights = [z['%s/w%d' % (meta['net'], k)] for k in range(2 * (meta['n_hidden'] + 1))]        # set_weights order
        self.layers = list(zip(self.weights[0::2], self.weights[1::2]))
        self.scale = z[meta['net'] + '/scale'] if meta['obs_scale'] else None
        self.w5, self.w_logp = tuple(float(v) for v in self['w5']), float(self['w_logp'])
        self.eps = self['eps'] if self.sampled else None

    def __getitem__(self, k):
        return self._z['%s/%s' % (self.name, k)]

    def ref_idx(self):
        return self._z[self.meta['rows'] + '/ref_idx'] if self.mode == 'training' else None

    def path_id(self):
        return self.meta['path_id'] if self.mode == 'selecting' else 0

    def net_args(self):
        """make_mlp's arguments (HostModel / DeviceModel)"""
        return self.dims + (self.hact, 'linear', self.layers, self.scale)

    def params64(self):
        return [self['g_params_64_%d' % k] for k in range(len(self.weights))]


def cases(task):
    z = golden(stem(task))
    return [Case(z, task, name, meta) for name, meta in json.loads(str(z['cases'])).items()]


def all_cases():
    return [c for task in TASKS for c in cases(task)]


def case_id(c):
    return '%s_%s' % (c.task, c.name)


WORST = {}                    # what -> the largest error / tolerance seen (the figures of DESIGN.md)


def _held(got, ref64, E, ok, what, key):
    """check_columns (it prints error / tolerance per column, then asserts) with the largest ratio noted under `key` first"""
    g = np.asarray(got, np.float64).reshape(len(ok), -1, len(E))[ok]
    r = np.asarray(ref64, np.float64).reshape(len(ok), -1, len(E))[ok]
    ratio = float((np.abs(g - r).max((0, 1)) / np.maximum(column_tolerance(E, ref64, ok), 1e-300)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    check_columns(got, ref64, E, ok, what)


def check_rows(c, g_obs0, g_actions, what):
    """g_obs0 [n, 9] and g_actions [steps, n, 2] against the float64 arrays, per column"""
    ok = c['ok']
    _held(g_obs0, c['g_obs0_64'], c['E_obs0'], ok, what + ' g_obs0', what + ' rows')
    _held(np.moveaxis(np.asarray(g_actions), 0, 1), np.moveaxis(c['g_actions_steps_64'], 0, 1), c['E_actions'], ok,
          what + ' g_actions', what + ' rows')


def check_params(c, tensors, what):
    """the parameter gradient, one array per layer tensor, against the float64 arrays: a tensor is one column of one row"""
    one = np.ones(1, bool)
    E = c['E_params']
    assert len(tensors) == len(c.weights)
    for k, (got, ref) in enumerate(zip(tensors, c.params64())):
        assert np.shape(got) == ref.shape, '%s: g_params[%d] has shape %s, the fixture %s' % (what, k, np.shape(got), ref.shape)
        _held(np.reshape(got, (1, -1, 1)), ref.reshape(1, -1, 1), E[k:k + 1], one, '%s g_params[%d]' % (what, k), what + ' params')
