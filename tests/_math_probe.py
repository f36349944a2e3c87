"""The test-only device probe: tests/_math_probe.hip compiled with the product's flags, and one call per operation with NumPy arrays in
and out.  Importing this module touches no device and compiles nothing; build_probe() compiles (once per session, into a pytest temporary
directory, the way _helpers.build_host_harness does) and Probe.run() is the first thing that opens the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from env_build_amd import build as eb_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, 'tests', '_math_probe.hip')

# the kernel's selector, in the order of _math_probe.hip:Op
OPS = ('sincos', 'sincos_k', 'atan', 'exp', 'elu', 'tanh', 'log', 'artanh', 'div_10', 'div_180', 'div_pi', 'div_26875', 'div_15625',
       'div_by', 'deg2rad', 'rad2deg', 'div', 'rcp', 'sqrt', 'u01', 'normal', 'f32_to_f16', 'f16_to_f32')
TWO_OUTPUTS = ('sincos', 'sincos_k', 'normal', 'f32_to_f16')
# the five divisors of the path (csrc/eb_device.h: C10, C180, CPi, C26875, C15625) by the operation that divides by them
DIVISORS = {'div_10': 10.0, 'div_180': 180.0, 'div_pi': float(np.float32(np.pi)), 'div_26875': 26.875, 'div_15625': 15.625}


class ProbeError(RuntimeError):
    """a HIP call of the probe failed (the text names it: `hipError`): the card may have faulted"""


def build_probe(tmp_path_factory):
    """tests/_math_probe.hip -> libmathprobe.so in a fresh temporary directory, with env_build_amd.build.FLAGS: the product's code generation"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = str(tmp_path_factory.mktemp('mathprobe') / 'libmathprobe.so')
    subprocess.check_call([hipcc] + eb_build.FLAGS + ['-shared', '-I', eb_build.CSRC, SOURCE, '-o', out])
    return Probe(out)


class Probe(object):
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.eb_math_probe_last_error.restype = C.c_char_p
        self.lib.eb_math_probe_run.restype = C.c_int
        self.lib.eb_math_probe_run.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        assert self.lib.eb_math_probe_op_count() == len(OPS)

    def run(self, op, a, b=None, c=None, P=0, rc=0.0):
        """operation `op` over the elements of a (and b, c) -> uint32 bit patterns: one array, or two for the operations of TWO_OUTPUTS"""
        arrs = [None if t is None else np.ascontiguousarray(t) for t in (a, b, c)]
        n = arrs[0].size
        assert all(t is None or (t.size == n and t.dtype.itemsize in (4, 8)) for t in arrs)
        o0 = np.zeros(n, np.uint32)
        o1 = np.zeros(n, np.uint32) if op in TWO_OUTPUTS else None
        args = []
        for t in arrs:
            args += [None, 0] if t is None else [t.ctypes.data_as(C.c_void_p), t.nbytes]
        rcode = self.lib.eb_math_probe_run(OPS.index(op), n, *args, int(P), float(rc), o0.ctypes.data_as(C.c_void_p),
                                           None if o1 is None else o1.ctypes.data_as(C.c_void_p))
        if rcode != 0:
            raise ProbeError('math probe %s: %s' % (op, self.lib.eb_math_probe_last_error().decode()))
        return o0 if o1 is None else (o0, o1)

    def f(self, op, x, **kw):
        """run() for the float -> float operations: float32 array in, uint32 bits out"""
        return self.run(op, np.ascontiguousarray(x, np.float32), **kw)
