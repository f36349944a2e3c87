"""Stream capture as a test instrument: what a C-ABI call enqueues on ONE stream, seen as the nodes of the hipGraph the capture
produced, and replayed.  A helper module like _tape.py and _policy.py: pytest does not collect it, and importing it touches no device
(torch and the HIP runtime are reached inside the functions that need them).

Route in use: PyTorch's own — torch.cuda.CUDAGraph(keep_graph=True), capture_begin(capture_error_mode='thread_local') on the side
stream, raw_cuda_graph() for the hipGraph_t, instantiate() / replay() for the launches.  The nodes are enumerated with
hipGraphGetNodes / hipGraphNodeGetType / hipGraphGetEdges through ctypes on the libamdhip64.so PyTorch has already loaded (opened by
its path inside torch/lib: the same mapping, no second runtime).

Every graph made here is what one stream recorded, i.e. a single chain; `is_chain()` says so from the graph's edges."""
import collections
import contextlib
import ctypes as C
import gc
import os

# hipGraphNodeType (hip_runtime_api.h)
_KIND = {0: 'kernel', 1: 'memcpy', 2: 'memset', 10: 'mem-alloc', 11: 'mem-free'}
_hip = None


class CaptureError(RuntimeError):
    pass


def hip_runtime():
    """the HIP runtime PyTorch loaded, with the few prototypes this module needs"""
    global _hip
    if _hip is None:
        import torch
        lib = C.CDLL(os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so'))
        lib.hipGraphGetNodes.restype = C.c_int
        lib.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        lib.hipGraphNodeGetType.restype = C.c_int
        lib.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        lib.hipGraphGetEdges.restype = C.c_int
        lib.hipGraphGetEdges.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        lib.hipGetErrorString.restype = C.c_char_p
        lib.hipGetErrorString.argtypes = [C.c_int]
        _hip = lib
    return _hip


def _check(rc, what):
    if rc != 0:
        raise CaptureError('%s: HIP error %d (%s)' % (what, rc, hip_runtime().hipGetErrorString(rc).decode()))


@contextlib.contextmanager
def no_collection():
    """The cyclic garbage collector held off for a captured region.  A collection that falls inside one may finalise a handle some earlier
    test left in a reference cycle (HostModel.__del__ -> eb_destroy: hipDeviceSynchronize, hipFree, hipStreamDestroy; MLPNet.__del__ ->
    eb_mlp_destroy: hipFree) — calls a capturing thread must not make, and the process has aborted from them.  torch.cuda.graph used to
    collect before it captured; since PyTorch 2.9 it does not (torch.compiler.config.force_cudagraph_gc).  Objects whose last reference
    goes inside the region are still freed there, as before: that is the code under capture, not the collector's timing."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def side_stream():
    import torch
    return torch.cuda.Stream()


class Captured(object):
    """one captured graph: node_types(), is_chain(), replay() on the stream it was captured on, close()"""

    def __init__(self, graph, stream, what):
        self._g, self.stream, self.what = graph, stream, what

    def _nodes(self):
        hip, g = hip_runtime(), C.c_void_p(self._g.raw_cuda_graph())
        n = C.c_size_t(0)
        _check(hip.hipGraphGetNodes(g, None, C.byref(n)), '%s: hipGraphGetNodes' % self.what)
        nodes = (C.c_void_p * max(1, n.value))()
        if n.value:
            _check(hip.hipGraphGetNodes(g, nodes, C.byref(n)), '%s: hipGraphGetNodes' % self.what)
        return [nodes[i] for i in range(n.value)]

    def node_types(self):
        """Counter over 'kernel' / 'memset' / 'memcpy' / 'mem-alloc' / 'mem-free' / 'other'"""
        hip, out = hip_runtime(), collections.Counter()
        for node in self._nodes():
            kind = C.c_int(-1)
            _check(hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)), '%s: hipGraphNodeGetType' % self.what)
            out[_KIND.get(kind.value, 'other')] += 1
        return out

    def is_chain(self):
        """n nodes, n - 1 edges, no node with two successors or two predecessors"""
        hip, g = hip_runtime(), C.c_void_p(self._g.raw_cuda_graph())
        n_nodes, n = len(self._nodes()), C.c_size_t(0)
        _check(hip.hipGraphGetEdges(g, None, None, C.byref(n)), '%s: hipGraphGetEdges' % self.what)
        if n.value != max(0, n_nodes - 1):
            return False
        if not n.value:
            return True
        src, dst = (C.c_void_p * n.value)(), (C.c_void_p * n.value)()
        _check(hip.hipGraphGetEdges(g, src, dst, C.byref(n)), '%s: hipGraphGetEdges' % self.what)
        return len(set(src[i] for i in range(n.value))) == n.value and len(set(dst[i] for i in range(n.value))) == n.value

    def replay(self):
        import torch
        if not getattr(self, '_ready', False):
            self._g.instantiate()
            self._ready = True
        with torch.cuda.stream(self.stream):
            self._g.replay()

    def close(self):
        if self._g is not None:
            self._g.reset()
            self._g = None


def capture(stream, fn, what='call'):
    """fn(raw_stream) recorded on `stream` (thread-local capture mode; nothing runs) -> Captured.  Whatever fn or the runtime raises, the
    capture is ended and the graph destroyed before CaptureError (naming `what`) leaves; the stream stays usable."""
    import torch
    g = torch.cuda.CUDAGraph(keep_graph=True)
    err = None
    with torch.cuda.stream(stream), no_collection():
        g.capture_begin(capture_error_mode='thread_local')
        try:
            fn(stream.cuda_stream)
        except Exception as e:                      # noqa: BLE001  (the entry's own error: reported below, after the capture has ended)
            err = e
        finally:
            try:
                g.capture_end()
            except Exception as e:                  # noqa: BLE001  (an invalidated capture: hipStreamEndCapture's error string is in e)
                err = err or e
    if err is not None:
        try:
            g.reset()
        except Exception:                           # noqa: BLE001
            pass
        raise CaptureError('%s: stream capture failed: %s: %s' % (what, type(err).__name__, err)) from err
    return Captured(g, stream, what)
