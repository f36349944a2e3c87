#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (container-only, like scripts/gen_golden_grad.py): the 'normalize' preprocessor's outputs from the reference's own
Python.

G22.  utils/preprocessor.py is imported UNMODIFIED over oracle/shim (oracle/refload's path rule); the stand-in tensorflow lacks
tf.Variable (with assign) and tf.ones, which RunningMeanStd touches for its TensorFlow mirrors: both are added to the imported shim
module here, at run time — oracle/ is not edited.  Every case is run twice through the reference's classes: on float32 inputs (the
reference's working precision: the env's observations and rewards are float32, so RunningMeanStd's moments and merge stay float32 —
`*_ref`) and on the same values as float64 with a float64 state (the yardstick — `*64`).

  tests/golden/g22_norm.npz          arrays and names only

  (1) obs_B<B>_D<D>/...   Preprocessor(D, num_agent=B).process_obs over 6 consecutive batches, B in {2, 65} x D in {1, 41}: x [6, B, D],
      y_ref (float32), y64, and the final (mean, var, count) of both runs.  Columns: |mean| / std from 0 to 10^3, one constant column
      (D = 41: column 39), one column with outliers that clip (the last).  clipob is 10 at B = 65 and 2 at B = 2: twelve samples cannot lie
      ten of their own standard deviations out.
  (2) rew1/...            process_rew(rew, done) on the num_agent=None branch as it stands: 40 steps with three dones; rew, done, r_ref,
      r64 and ret_rms (mean, var, count) after every step, both runs.  It pins the recursion, the update-before-scale order and the reset
      through n = 1.
  (3) rewB/...            B = 65, 6 steps.  The reference's batched branch RAISES as written — preprocessor.py:88 hands np.zeros the
      array as a shape — so the three-line recursion is written out HERE, around the reference's own ret_rms.update and
      np_process_rewards:   ret = ret * gamma + rew;  ret_rms.update(ret);  r = np_process_rewards(rew);  ret = where(done, 0, ret)

No clipped element is the only evidence for a column, and at most a quarter of any case's elements sit at the clip: asserted below.

    python scripts/gen_golden_norm.py            # rewrite the fixture
    python scripts/gen_golden_norm.py --check    # regenerate in memory and compare with the committed file
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'g22_norm.npz')
MAX_BYTES = 1 << 20
GAMMA, EPSILON, CLIPREW = 0.99, 1e-8, 10.0
BATCHES = 6


def reference():
    """the reference's utils.preprocessor, with tf.Variable and tf.ones added to the stand-in tensorflow"""
    for p in (refload.SHIM, refload.REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tensorflow as tf

    class Variable(object):
        def __init__(self, value, dtype=None, trainable=False):
            self.value = value

        def assign(self, value):
            self.value = value

    tf.Variable = Variable
    tf.ones = lambda shape, dtype=np.float32: tf.Tensor(np.ones(shape, dtype=dtype))
    from utils import preprocessor
    return preprocessor


def in_double(pre):
    """the reference's Preprocessor with a float64 state: fed float64 inputs it then computes in float64 throughout"""
    for rms in (pre.ob_rms, pre.ret_rms):
        if rms is not None:
            rms.mean, rms.var = rms.mean.astype(np.float64), rms.var.astype(np.float64)
    return pre


def obs_batches(B, D, rng):
    """x [BATCHES, B, D] float32 and the clip"""
    n = BATCHES * B
    if D == 1:
        x = 50.0 + 5.0 * rng.standard_normal((n, 1))
    else:
        ratio = np.concatenate([[0.0], np.logspace(-1, 3, D - 3)])          # |mean| / std of the columns 0 .. D - 3
        std = np.logspace(-2, 2, D - 2)[rng.permutation(D - 2)]
        sign = np.where(rng.random(D - 2) < 0.5, -1.0, 1.0)
        x = np.empty((n, D))
        x[:, :D - 2] = sign * ratio * std + std * rng.standard_normal((n, D - 2))
        x[:, D - 2] = 3.25                                                   # the constant column
        x[:, D - 1] = 2.0 + rng.standard_normal(n)
    if B >= 8:                                                               # outliers, in the later batches, in the last column
        rows = rng.choice(np.arange(2 * B, n), 4, replace=False)
        x[rows, D - 1] += 60.0 * x[:, D - 1].std()
    return x.reshape(BATCHES, B, D).astype(np.float32), (10.0 if B >= 8 else 2.0)


def clipped_share(y, clip, per_column=True):
    at = np.abs(y) >= clip
    assert at.mean() <= 0.25, at.mean()
    if per_column:
        assert (~at).reshape(-1, y.shape[-1]).any(axis=0).all()             # every column has evidence that is not a clip
    return int(at.sum())


def generate():
    P = reference()
    rng = np.random.default_rng(22)
    out = {'gamma': np.float64(GAMMA), 'epsilon': np.float64(EPSILON)}
    for B in (2, 65):
        for D in (1, 41):
            x, clip = obs_batches(B, D, rng)
            ref = P.Preprocessor((D,), clipob=clip, gamma=GAMMA, epsilon=EPSILON, num_agent=B)
            dbl = in_double(P.Preprocessor((D,), clipob=clip, gamma=GAMMA, epsilon=EPSILON, num_agent=B))
            y_ref = np.stack([ref.process_obs(x[k]) for k in range(BATCHES)])
            y64 = np.stack([dbl.process_obs(x[k].astype(np.float64)) for k in range(BATCHES)])
            assert y_ref.dtype == np.float32 and y64.dtype == np.float64
            n_clip = clipped_share(y64, clip)
            assert (B < 8) or n_clip > 0
            key = 'obs_B%d_D%d/' % (B, D)
            out.update({key + 'x': x, key + 'clip': np.float64(clip), key + 'y_ref': y_ref, key + 'y64': y64})
            for tag, pre in (('ref', ref), ('64', dbl)):
                mean, var, count = pre.ob_rms.get_params()
                out.update({key + 'mean_' + tag: np.asarray(mean), key + 'var_' + tag: np.asarray(var), key + 'count_' + tag: np.float64(count)})
    # (2) one env, the branch as it stands
    steps = 40
    rew = (-3.0 + 40.0 * rng.standard_normal(steps)).astype(np.float32)
    done = np.zeros(steps, np.uint8)
    done[[9, 10, 31]] = 1
    ref = P.Preprocessor((1,), gamma=GAMMA, epsilon=EPSILON, cliprew=CLIPREW)
    dbl = in_double(P.Preprocessor((1,), gamma=GAMMA, epsilon=EPSILON, cliprew=CLIPREW))
    rows = {k: [] for k in ('r_ref', 'r64', 'rms_ref', 'rms64')}
    for t in range(steps):
        rows['r_ref'].append(ref.process_rew(rew[t], bool(done[t])))
        rows['rms_ref'].append([float(v) for v in ref.ret_rms.get_params()])
        rows['r64'].append(dbl.process_rew(np.float64(rew[t]), bool(done[t])))
        rows['rms64'].append([float(v) for v in dbl.ret_rms.get_params()])
    r_ref, r64 = np.asarray(rows['r_ref']), np.asarray(rows['r64'], np.float64)
    assert r_ref.dtype == np.float32, r_ref.dtype
    clipped_share(r64, CLIPREW, per_column=False)
    out.update({'rew1/rew': rew, 'rew1/done': done, 'rew1/r_ref': r_ref, 'rew1/r64': r64, 'rew1/rms_ref': np.asarray(rows['rms_ref'], np.float64),
                'rew1/rms64': np.asarray(rows['rms64'], np.float64)})
    # (3) B envs: the recursion written out around the reference's own update and scaling (its batched branch raises)
    B, steps = 65, 6
    rew = (-3.0 + 40.0 * rng.standard_normal((steps, B))).astype(np.float32)
    done = (rng.integers(0, 8, (steps, B)) * (rng.random((steps, B)) < 0.2)).astype(np.uint8)        # done codes 0 .. 7
    try:
        P.Preprocessor((1,), num_agent=B).process_rew(rew[0], done[0])
        raise AssertionError('the batched branch no longer raises: use it')
    except (TypeError, ValueError):                                       # np.zeros(<float array>): not a shape
        pass
    res = {}
    for tag, dtype in (('ref', np.float32), ('64', np.float64)):
        pre = P.Preprocessor((1,), gamma=GAMMA, epsilon=EPSILON, cliprew=CLIPREW, num_agent=B)
        if dtype is np.float64:
            in_double(pre)
        ret, rs = np.zeros(B, dtype), []
        for t in range(steps):
            ret = ret * pre.gamma + rew[t].astype(dtype)
            pre.ret_rms.update(ret)
            rs.append(pre.np_process_rewards(rew[t].astype(dtype)))
            ret = np.where(done[t] != 0, np.zeros_like(ret), ret)
        assert ret.dtype == dtype and rs[0].dtype == dtype
        res[tag] = (np.stack(rs), ret, np.asarray([float(v) for v in pre.ret_rms.get_params()]))
    clipped_share(res['64'][0], CLIPREW, per_column=False)
    out.update({'rewB/rew': rew, 'rewB/done': done, 'rewB/r_ref': res['ref'][0], 'rewB/r64': res['64'][0], 'rewB/ret_ref': res['ref'][1],
                'rewB/ret64': res['64'][1], 'rewB/rms_ref': res['ref'][2], 'rewB/rms64': res['64'][2]})
    return out


def main():
    out = generate()
    if '--check' in sys.argv:
        have = np.load(GOLD)
        assert sorted(have.files) == sorted(out), 'the fixture holds other arrays'
        for k in out:
            assert np.array_equal(have[k], out[k], equal_nan=True), k
        print('%s: %d arrays equal' % (GOLD, len(out)))
        return
    np.savez(GOLD, **out)
    size = os.path.getsize(GOLD)
    assert size < MAX_BYTES, size
    print('%s: %d arrays, %d bytes' % (GOLD, len(out), size))


if __name__ == '__main__':
    main()
