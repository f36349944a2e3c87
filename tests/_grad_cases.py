"""Shared by tests/test_grad_host.py and tests/test_gpu_grad.py: the gradient fixtures (scripts/gen_golden_grad.py) and the
tolerance they carry.

Tolerance (per output column c, over the rows whose flag is set):
    |g - g_float64_ref| <= 4 * E_c + 2**-20 * max_rows |g_float64_ref[:, c]|,   E_c = max_rows |g_float32_ref - g_float64_ref|
The code under test is a second, independent fp32 evaluation of the reference's expressions (its own operation order, its own
sin / cos), so its error is of the size of the reference's own fp32 error; the factor covers a sample maximum over a few hundred
rows; the floor is eight fp32 ulps of the column's magnitude, for columns where the reference's two runs happen to agree.
At most 1 % of a file's rows may carry a cleared flag (a condition on the inputs, not a measurement)."""
import json

import numpy as np

from tests._helpers import golden

TASKS = ('left', 'straight', 'right')
MAX_EXCLUDED = 0.01


class Case(object):
    def __init__(self, z, name, meta):
        self.name, self.meta = name, meta
        self.mode, self.n_veh, self.n_future, self.path_id = meta['mode'], meta['n_veh'], meta['n_future'], meta['path_id']
        self.nd = 9 + 3 * self.n_future
        self._z = z

    def __getitem__(self, k):
        return self._z['%s/%s' % (self.name, k)]

    def ref_idx(self):
        return self['ref_idx'] if self.mode == 'training' else None


def cases(kind, task):
    """kind: 'g15_grad_step' / 'g16_grad_chain' -> list of Case"""
    z = golden('%s_%s' % (kind, task))
    return [Case(z, name, meta) for name, meta in json.loads(str(z['cases'])).items()]


def column_tolerance(E, ref64, ok):
    ref = np.abs(np.asarray(ref64, np.float64).reshape(len(ok), -1, len(E)))[ok]
    return 4.0 * np.asarray(E, np.float64) + 2.0 ** -20 * ref.max((0, 1))


def check_columns(got, ref64, E, ok, what, ratios=None):
    """got / ref64: [B, C] (or [B, H, C]: every step of a row held to column c's bound); -> max |got - ref| / E per column"""
    got = np.asarray(got, np.float64).reshape(len(ok), -1, len(E))[ok]
    ref = np.asarray(ref64, np.float64).reshape(len(ok), -1, len(E))[ok]
    err = np.abs(got - ref).max((0, 1))
    tol = column_tolerance(E, ref64, ok)
    ratio = err / np.maximum(np.asarray(E, np.float64), 1e-300)
    fmt = lambda v: np.array2string(np.asarray(v), precision=2, max_line_width=100000)
    print('%-58s max|g - g64| / E per column: %s   err / tolerance: %s' % (
        what, fmt(np.where(np.asarray(E) > 0, ratio, np.nan)), fmt(err / np.maximum(tol, 1e-300))))
    if ratios is not None:
        ratios[what] = ratio
    assert np.isfinite(got).all(), '%s: non-finite gradient' % what
    assert (err <= tol).all(), '%s: columns %s exceed 4 E + 2^-20 max|g|: err %s, tol %s' % (what, np.nonzero(err > tol)[0], err, tol)
