"""TEST INFRASTRUCTURE — a stand-in for the `tensorflow` symbols the reference's dynamics_and_models.py uses, over torch tensors
with autograd on (scripts/gen_golden_grad.py; never imported by env_build_amd/).

The same job as oracle/shim/tensorflow (NumPy), plus gradients: `stop_gradient` is `detach`, the floating dtype is switchable
(set_dtype: float64 for the yardstick, float32 for the reference's own working precision), and every data-dependent decision —
the condition of a `where`, both sides of a `clip_by_value`, the result of an `argmin` — is appended to DECISIONS so that two runs
can be compared row by row.  Python / NumPy scalars take the tensor's dtype, as TensorFlow's operator overloads do.
"""
import contextlib

import numpy as np
import torch

_DT = [torch.float64]
DECISIONS = []          # tensors whose leading dimension is the batch (others are recorded too; the reader filters)
float32 = 'float'       # tf.float32: "the working precision"
int32 = torch.int32
int64 = torch.int64


def set_dtype(dt):
    _DT[0] = dt


def _unwrap(x):
    return x.t if isinstance(x, Tensor) else x


def _tt(x):
    """anything -> torch tensor; floating values in the working precision"""
    x = _unwrap(x)
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    return x.to(_DT[0]) if x.dtype.is_floating_point and x.dtype != _DT[0] else x


class Tensor(object):
    __array_ufunc__ = None      # NumPy operands defer to the reflected operators below
    __hash__ = None

    def __init__(self, t):
        self.t = _tt(t)

    shape = property(lambda s: tuple(s.t.shape))
    dtype = property(lambda s: s.t.dtype)

    def numpy(self): return self.t.detach().numpy()
    def __len__(self): return self.t.shape[0]
    def __float__(self): return float(self.t)
    def __int__(self): return int(self.t)
    __index__ = __int__
    def __bool__(self): return bool(self.t)

    def __getitem__(self, k):
        k = _unwrap(k)
        return Tensor(self.t[torch.as_tensor(k) if isinstance(k, np.ndarray) else k])

    def _op(self, other, fn, swap=False):
        o = _unwrap(other)
        if isinstance(o, np.ndarray):
            o = _tt(o)
        elif not isinstance(o, torch.Tensor) and self.t.dtype.is_floating_point:
            o = torch.tensor(float(o), dtype=self.t.dtype)
        return Tensor(fn(o, self.t) if swap else fn(self.t, o))

    def __neg__(self): return Tensor(-self.t)


for _name, _fn in (('add', torch.add), ('sub', torch.sub), ('mul', torch.mul), ('truediv', torch.div)):
    setattr(Tensor, '__%s__' % _name, lambda s, o, f=_fn: s._op(o, f))
    setattr(Tensor, '__r%s__' % _name, lambda s, o, f=_fn: s._op(o, f, True))
for _name, _fn in (('lt', torch.lt), ('le', torch.le), ('gt', torch.gt), ('ge', torch.ge), ('eq', torch.eq), ('ne', torch.ne)):
    setattr(Tensor, '__%s__' % _name, lambda s, o, f=_fn: s._op(o, f))


def convert_to_tensor(x, dtype=None):
    t = _tt(x)
    return Tensor(t if dtype in (None, float32) else t.to(dtype))


constant = convert_to_tensor


def cast(x, dtype):
    return convert_to_tensor(x, dtype)


def square(x): return Tensor(_tt(x) ** 2)
def sqrt(x): return Tensor(torch.sqrt(_tt(x)))
def sin(x): return Tensor(torch.sin(_tt(x)))
def cos(x): return Tensor(torch.cos(_tt(x)))
def atan(x): return Tensor(torch.atan(_tt(x)))
def zeros_like(x): return Tensor(torch.zeros_like(_tt(x)))
def zeros(shape, dtype=None): return Tensor(torch.zeros(tuple(shape), dtype=_DT[0]))
def stop_gradient(x): return Tensor(_tt(x).detach())
def stack(xs, axis=0): return Tensor(torch.stack([_tt(x) for x in xs], axis))
def concat(xs, axis): return Tensor(torch.cat([_tt(x) for x in xs], axis))
def tile(x, multiples): return Tensor(_tt(x).repeat(*[int(m) for m in _tt(multiples).tolist()]))
def reshape(x, shape): return Tensor(_tt(x).reshape(tuple(shape)))
def shape(x): return Tensor(torch.tensor(list(_tt(x).shape), dtype=torch.int32))
def expand_dims(x, axis): return Tensor(_tt(x).unsqueeze(axis))
def gather(params, indices): return Tensor(_tt(params)[_tt(indices).long()])
def logical_and(a, b): return Tensor(torch.logical_and(_tt(a), _tt(b)))


def where(cond, x, y):
    c = _tt(cond)
    DECISIONS.append(c.detach().clone())
    x, y = _unwrap(x), _unwrap(y)
    tensors = [v for v in (x, y) if isinstance(v, (torch.Tensor, np.ndarray))]
    like = _tt(tensors[0])
    x, y = (_tt(v) if isinstance(v, (torch.Tensor, np.ndarray)) else torch.as_tensor(v, dtype=like.dtype) for v in (x, y))
    return Tensor(torch.where(c, x, y))


def argmin(x, axis):
    i = torch.argmin(_tt(x), axis)
    DECISIONS.append(i.clone())
    return Tensor(i)


def clip_by_value(x, lo, hi):
    t = _tt(x)
    DECISIONS.append((t < lo).detach())
    DECISIONS.append((t > hi).detach())
    return Tensor(torch.clamp(t, lo, hi))       # cotangent passes where lo <= x <= hi, as tf.clip_by_value's does


@contextlib.contextmanager
def name_scope(name):
    yield name


def function(fn=None, **kwargs):
    return (lambda f: f) if fn is None else fn


class TensorSpec(object):
    def __init__(self, *a, **k):
        pass


class _Threading(object):
    set_inter_op_parallelism_threads = staticmethod(lambda n: None)
    set_intra_op_parallelism_threads = staticmethod(lambda n: None)


class _Experimental(object):
    set_visible_devices = staticmethod(lambda devices, kind=None: None)


class _Config(object):
    threading = _Threading()
    experimental = _Experimental()


config = _Config()
