"""Shared by tests/test_per_host.py and tests/test_gpu_per.py (a helper module like _offpolicy.py: pytest does not collect it, and importing
it touches no device): the prioritised-replay library built and bound, the capacities every property is held at, and the hand-made cases
— the exact prefix boundaries, the fallback, the lone last leaf, the write-back's rows — with what they must give, computed once."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import per as P
from tests._epoch import struct_fields
from tests._helpers import ROOT
from tests._offpolicy import bits  # noqa: F401

HEADER = os.path.join(ROOT, 'include', 'envbuild_per.h')
KERNELS = ('per_repair_range_kernel', 'per_repair_rows_kernel', 'per_repair_top_kernel', 'per_reset_kernel', 'per_sample_kernel',
           'per_set_range_kernel', 'per_stamp_kernel', 'per_weigh_kernel', 'per_write_kernel')
ENTRIES = ('eb_per_reset', 'eb_per_set', 'eb_per_sample', 'eb_per_weigh')
STRUCTS = {'eb_per_reset_args': P.EbPerResetArgs, 'eb_per_set_args': P.EbPerSetArgs, 'eb_per_sample_args': P.EbPerSampleArgs,
           'eb_per_weigh_args': P.EbPerWeighArgs}
STRUCT_OF = dict(zip(ENTRIES, STRUCTS))
UNIT = ('eb_per.hip', 'eb_per.h', 'eb_per_device.h')
CAPACITIES = (1, 2, 31, 32, 33, 1023, 1024, 1025, 32769)                # the issue's list: every level count 1 .. 4 and a big level
SENTINEL = -77.25


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def fields_of(src, name):
    return struct_fields(src, name, nested={'uint32_t': C.c_uint32})


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_per.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, bytes)"""
    path = eb_build.build_per()
    assert not eb_build.per_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.per_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in P.PER_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


def header_levels(C_):
    """the header's formula, written out once more and independently of per.tree_levels: n_k = ceil(C / 32^k) up to the level with one
    node, off_1 = 0, off_(k+1) = off_k + n_k -> (n[1:], off[1:], doubles)"""
    n, k = [], 1
    while True:
        n.append((C_ + 32 ** k - 1) // 32 ** k)
        if n[-1] == 1:
            break
        k += 1
    off = [sum(n[:i]) for i in range(len(n))]
    return n, off, sum(n)


def tree_by_loops(prio):
    """the invariant with plain Python loops and Python floats (IEEE doubles): level by level, each node the ascending sum from 0.0"""
    level, out = [float(x) for x in np.asarray(prio, np.float32)], []
    while True:
        up = []
        for i in range(0, len(level), 32):
            s = 0.0
            for x in level[i:i + 32]:
                s = s + x
            up.append(s)
        out += up
        level = up
        if len(up) == 1:
            return np.array(out, np.float64)


@functools.lru_cache(maxsize=None)
def leaves(C_, seed=0):
    """priorities over C_ slots as after some training: about a third never set (0, interleaved), the rest spread over eight decades"""
    rng = np.random.default_rng(100 + C_ + seed)
    p = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), C_)).astype(np.float32)
    p[rng.uniform(size=C_) < 0.33] = 0
    p[rng.integers(0, C_)] = np.float32(0.75)                            # at least one positive leaf
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def boundary_case(C_):
    """Every prefix boundary of a ring, exactly.  Leaves are integers in {0, 2, 3, 4, 5}, so every partial sum in any order is an exact
    double and the hierarchy must give what one flat cumulative sum gives.  m = total rows make t = total / m = 1.0, so u = (double)r +
    U_r with no further rounding.  With B_i the prefix up to and including leaf i: row B_i - 1 gets U = 1 - (one double step below B_i),
    i.e. u is the double just below B_i; row B_i (when there is one) gets U = 0, u = B_i itself; every other row U = 0.5.  priorities >= 2
    keep the two rows of a boundary apart.  -> (prio, u_in, the index each row must draw)"""
    rng = np.random.default_rng(7 + C_)
    prio = rng.choice(np.array([0, 2, 3, 4, 5], np.float32), C_)
    prio[rng.integers(0, C_)] = 3
    B = np.cumsum(prio.astype(np.float64))
    m = int(B[-1])
    u_in = np.full(m, 0.5)
    ends = B[prio > 0]
    below = np.nextafter(ends, -np.inf)
    u_in[ends.astype(np.int64) - 1] = below - (ends - 1.0)
    at = ends[ends < m].astype(np.int64)
    u_in[at] = 0.0
    u = np.arange(m, dtype=np.float64) + u_in
    assert np.array_equal(u[ends.astype(np.int64) - 1], below) and (u_in >= 0).all() and (u_in < 1).all()
    want = np.searchsorted(B, u, side='right').astype(np.int32)        # the first leaf whose prefix exceeds u
    assert (prio[want] > 0).all()
    assert np.array_equal(want[ends.astype(np.int64) - 1], np.flatnonzero(prio > 0))                  # just below B_i: leaf i
    nxt = np.flatnonzero(prio > 0)[1:]
    assert np.array_equal(want[at], nxt)                                # at B_i: the next positive leaf
    for a in (prio, u_in, want):
        a.setflags(write=False)
    return prio, u_in, want


@functools.lru_cache(maxsize=None)
def fallback_case(C_):
    """A node whose STORED sum exceeds what its children reach — what rounding could leave behind, made large by hand: the tree is
    tree_reference's except that the first level-1 node with a positive leaf, and every ancestor up to the root, is raised by that node's
    true sum.  One draw, aimed through u_in into the excess, runs past the node's last child at the leaf level and must land on the LAST
    POSITIVE leaf of that node.  -> (prio, tree, u_in [1], the index)"""
    prio = leaves(C_, seed=1).copy()
    n, off, _ = P.tree_levels(C_)
    tree = P.tree_reference(prio)
    node = int(np.flatnonzero(tree[:n[1]] > 0)[0])
    kids = prio[32 * node:32 * node + 32]
    last = 32 * node + int(np.flatnonzero(kids > 0)[-1])
    excess = float(tree[node])                                           # the stored sum becomes twice the true one
    before = float(tree[:node].sum())                                    # 0.0: the nodes before it hold no positive leaf
    assert before == 0.0
    i = node
    for k in range(1, len(n)):
        tree[off[k] + i] += excess
        i //= 32
    total = tree[-1]
    u = 1.75 * excess                                                    # inside the raised node, beyond the 1.0 * excess its leaves reach
    u_in = np.array([u / total])
    assert 0 <= u_in[0] < 1 and excess < u_in[0] * total < 2 * excess
    return prio, tree, u_in, last


def write_back_rows(C_, m, kind, seed=0):
    """(index int32 [m], value float32 [m]) for the indexed route: 'random' — indices over the ring with repeats and, every seventh row,
    one of the rows that must be skipped or clamped (index -1 and C, value NaN, 0, -1, inf, below and above the clamp); 'one' — every
    row names one leaf; 'twice' — every leaf named twice (m = 2 C)"""
    rng = np.random.default_rng(5000 + C_ + 13 * m + seed)
    value = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), m)).astype(np.float32)
    if kind == 'one':
        return np.full(m, C_ // 2, np.int32), value
    if kind == 'twice':
        idx = np.concatenate([rng.permutation(C_), rng.permutation(C_)]).astype(np.int32)
        return idx, np.exp(rng.uniform(np.log(1e-3), np.log(1e3), 2 * C_)).astype(np.float32)
    idx = rng.integers(0, C_, m).astype(np.int32)
    odd = [(-1, 1.0), (C_, 1.0), (0, np.nan), (0, 0.0), (C_ - 1, -1.0), (0, np.inf), (C_ - 1, 2.0 ** -60), (0, 2.0 ** 60), (C_ - 1, -np.inf)]
    for r in range(0, m, 7):
        j, v = odd[(r // 7) % len(odd)]
        idx[r], value[r] = j, v
    return idx, value


def weigh_rows(m, seed=0, nan=False, undrawn=False):
    """what eb_per_weigh reads for m rows: index (>= 0, or -1 every ninth row with `undrawn`), prio (positive, -> NaN where -1),
    min_partials (their per-block minima, as eb_per_sample leaves them), q1, q2, y (NaN TD errors every eleventh row with `nan`),
    g_q1, g_q2, loss1, loss2"""
    rng = np.random.default_rng(900 + m + seed)
    index = rng.integers(0, 1000, m).astype(np.int32)
    prio = np.exp(rng.uniform(np.log(2.0 ** -40), np.log(2.0 ** 40), m)).astype(np.float32)
    if undrawn:
        index[::9] = -1
        prio[::9] = np.nan
    partials = np.full(64, np.inf, np.float32)
    block = (np.arange(m) // 256) % 64
    for b in range(64):
        sel = (block == b) & (index >= 0)
        if sel.any():
            partials[b] = prio[sel].min()
    rows = {k: (3.0 * rng.standard_normal(m)).astype(np.float32) for k in ('q1', 'q2', 'y', 'g_q1', 'g_q2', 'loss1', 'loss2')}
    if nan:
        rows['q1'][::11] = np.nan
        rows['y'][5::11] = np.nan
    return dict(index=index, prio=prio, min_partials=partials, **rows)
