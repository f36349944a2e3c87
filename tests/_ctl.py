"""Shared by tests/test_ctl_host.py and tests/test_gpu_ctl.py (a helper module like _epoch.py and _collect.py: pytest does not collect it,
and importing it touches no device): the control library built and bound, the header's structs as ctypes field lists, the log-probability
rows of the KL cases, a control block on the device cut from the middle of a larger allocation, and the PPOEpochs case of the stop test."""
import ctypes as C
import functools
import os
import re

import numpy as np

from env_build_amd import build as eb_build
from env_build_amd import ctl, train
from tests import _epoch as E
from tests._helpers import ROOT

HEADER = os.path.join(ROOT, 'include', 'envbuild_ctl.h')
KERNELS = ('adam_norm_ctl_kernel', 'adam_update_ctl_kernel', 'ctl_begin_kernel', 'kl_fold_kernel', 'kl_partial_kernel')
ENTRIES = ('eb_ctl_begin', 'eb_kl_stop', 'eb_adam_step_ctl')
UNIT = ('eb_ctl.hip', 'eb_ctl.h', 'eb_ctl_device.h')
SCALARS = dict(E.SCALARS, uint32_t=C.c_uint32)
KL_SIZES = (1, 255, 256, 257, 16384, 16385)
SENTINEL = -77.25

# the PPOEpochs case of the stop test: tests/_epoch's networks and data, 2 epochs x 2 minibatches of 64 rows
ROWS, EPOCHS, MINIBATCHES = 64, 2, 2
SLOTS = EPOCHS * MINIBATCHES
N = MINIBATCHES * ROWS + 3


def header():
    """(the header's text, the same without comments)"""
    with open(HEADER) as fh:
        text = fh.read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def struct_fields(src, name, nested=()):
    """`typedef struct name { ... } name;` -> [(field, ctype)] in order; a pointer is c_void_p; the columns of a declaration may be
    padded with blanks"""
    nested = dict(nested)
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), src, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.match(r'(.*?)(\w+)$', decl)
        kind = m.group(1).replace('const ', '').strip()
        fields.append((m.group(2), C.c_void_p if kind.endswith('*') else nested[kind] if kind in nested else SCALARS[kind]))
    return fields


@functools.lru_cache(maxsize=None)
def library():
    """libenvbuild_ctl.so built from the tree (hipcc --offload-arch=gfx950 cross-compiles without a GPU) and bound -> (CDLL, its bytes)"""
    path = eb_build.build_ctl()
    assert not eb_build.ctl_needs_build()
    with open(path + '.srchash') as fh:
        assert fh.read().strip() == eb_build.ctl_source_hash()
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(path)
    for name, (res, args) in ctl.CTL_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    with open(path, 'rb') as fh:
        return lib, fh.read()


@functools.lru_cache(maxsize=None)
def kl_rows(n):
    """logp and logp_old of n rows: differences of a few hundredths in both directions, mean about +0.01"""
    rng = np.random.default_rng(27 + n)
    logp_old = (-2.0 + rng.standard_normal(n)).astype(np.float32)
    logp = (logp_old - np.float32(0.01) + np.float32(0.05) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return logp, logp_old


def kl_of(logp, logp_old):
    """fold_log's approx_kl of the rows, from ppo_log_reference: the yardstick of eb_kl_stop"""
    from env_build_amd import epoch
    return float(epoch.fold_log(epoch.ppo_log_reference(logp=logp, logp_old=logp_old))['approx_kl'])


def ctl_bytes(d):
    """a dict of the six fields -> the 32 bytes of an eb_update_ctl"""
    c = ctl.EbUpdateCtl(iteration=d['iteration'], lr_scale=float(d['lr_scale']), stopped=d['stopped'], slot=d['slot'],
                        stopped_at=d['stopped_at'], last_kl=d['last_kl'])
    return np.frombuffer(bytes(c), np.uint8).copy()


class Block(object):
    """an eb_update_ctl on the device in the MIDDLE of a larger allocation, sentinel int64s on both sides; host() -> (the six fields,
    whether the slack is as made)"""
    SLACK, FILL = 3, -77

    def __init__(self, fields=None):
        import torch
        self.big = torch.full((4 + 2 * self.SLACK,), self.FILL, dtype=torch.int64, device='cuda')
        self.view = self.big[self.SLACK:self.SLACK + 4]
        self.set(fields)

    def set(self, fields=None):
        import torch
        raw = np.zeros(32, np.uint8) if fields is None else ctl_bytes(fields)
        self.view.copy_(torch.from_numpy(raw.view(np.int64).copy()).cuda())
        torch.cuda.synchronize()

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        import torch
        torch.cuda.synchronize()
        raw = self.big.cpu().numpy()
        ok = bool((raw[:self.SLACK] == self.FILL).all() and (raw[self.SLACK + 4:] == self.FILL).all())
        return ctl._fields_of(raw[self.SLACK:self.SLACK + 4].copy().view(np.uint8)), ok


def live(scale=1.0, stopped=0, iteration=1, slot=0, stopped_at=-1, last_kl=0.0):
    """the six fields of a block inside an iteration"""
    return dict(iteration=iteration, lr_scale=np.float32(scale), stopped=stopped, slot=slot, stopped_at=stopped_at, last_kl=last_kl)


def same_ctl(got, want):
    """two dicts of the six fields, bit for bit (a NaN last_kl equals a NaN)"""
    return all(np.array_equal(np.asarray(got[k]).reshape(1), np.asarray(want[k]).reshape(1), equal_nan=True) for k in ctl.FIELDS)


# ---- Adam segments ---------------------------------------------------------------------------------------------------------------------------
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8
GAP = 3                                                            # floats between two segments: odd offsets, 4-byte alignment only
LAYOUTS = ((1,), (1023,), (1024,), (1025,), (5, 0, 2049), (262145,))   # the last: 257 chunks, more than the 256 partials


@functools.lru_cache(maxsize=None)
def adam_inputs(counts, steps=2):
    """per segment: parameters N(0, 1), and `steps` gradients spread over four decades"""
    rng = np.random.default_rng(len(counts) * 1000 + sum(counts))
    p0 = [rng.standard_normal(c).astype(np.float32) for c in counts]
    grads = [[(rng.standard_normal(c) * 10.0 ** rng.uniform(-3.0, 1.0, c)).astype(np.float32) for c in counts] for _ in range(steps)]
    return p0, grads


class Segments(object):
    """p, g, m, v for every segment, cut from ONE buffer each at odd offsets with GAP sentinel floats between them; the Adam state in the
    middle of sentinel int64s."""

    def __init__(self, counts, p0):
        import torch
        self.counts = counts
        self.at, at = [], 1
        for c in counts:
            self.at.append(at)
            at += c + GAP
        self.size = at
        self.buf = {k: torch.full((self.size,), SENTINEL, device='cuda') for k in 'pgmv'}
        for a, c, p in zip(self.at, counts, p0):
            self.buf['p'][a:a + c] = torch.from_numpy(p).cuda()
            self.buf['m'][a:a + c] = 0.0
            self.buf['v'][a:a + c] = 0.0
        self.state_big = torch.full((4 + 2 * Block.SLACK,), Block.FILL, dtype=torch.int64, device='cuda')
        self.state = self.state_big[Block.SLACK:Block.SLACK + 4]
        self.state.zero_()
        self.partials = torch.zeros(train.EB_TRAIN_ADAM_PARTIALS, dtype=torch.float64, device='cuda')

    def set_grads(self, grads):
        import torch
        for a, c, g in zip(self.at, self.counts, grads):
            self.buf['g'][a:a + c] = torch.from_numpy(g).cuda()
        torch.cuda.synchronize()                                   # the fills are on the null stream; a side stream does not wait for it

    def fill(self, a, lr=LR, wd=0.0, max_norm=0.0, stream=None):
        """an eb_adam_args (a struct of its own, or the `adam` member of an eb_adam_ctl_args) filled in place"""
        a.n_segments, a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_grad_norm = len(self.counts), lr, BETAS[0], BETAS[1], EPS, wd, max_norm
        a.state, a.partials, a.stream = self.state.data_ptr(), self.partials.data_ptr(), stream
        for k, (at, c) in enumerate(zip(self.at, self.counts)):
            seg = a.segments[k]
            seg.params, seg.grads, seg.m, seg.v = (self.buf[name].data_ptr() + 4 * at for name in 'pgmv')
            seg.count = c
        return a

    def host(self):
        """every byte this harness owns: the four buffers whole (segments and gaps), the state with its slack"""
        import torch
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in self.buf.items()}
        out['state'] = self.state_big.cpu().numpy()
        return out

    def gaps_untouched(self, host):
        inside = np.zeros(self.size, bool)
        for a, c in zip(self.at, self.counts):
            inside[a:a + c] = True
        slack = np.r_[host['state'][:Block.SLACK], host['state'][Block.SLACK + 4:]]
        return all((host[k][~inside] == SENTINEL).all() for k in 'pgmv') and bool((slack == Block.FILL).all())


# ---- the PPOEpochs case ---------------------------------------------------------------------------------------------------------------------
def epochs_case(controlled, data_of=None, **control_kw):
    """(loop, update) on tests/_epoch's networks and data, 2 epochs x 2 minibatches of 64 rows under the keyed shuffle: a ctl.PPOEpochs
    over a ctl.PPOUpdate when `controlled`, the plain epoch.PPOEpochs over a train.PPOUpdate otherwise"""
    from env_build_amd import epoch
    policy, value = E.make_nets()
    data = E.make_data(policy, n=N)
    if controlled:
        upd = ctl.PPOUpdate(policy, value, ROWS, **dict(E.PPO_KW, **control_kw))
        return ctl.PPOEpochs(upd, data, EPOCHS, MINIBATCHES, seed=E.SEED), upd
    upd = train.PPOUpdate(policy, value, ROWS, **E.PPO_KW)
    return epoch.PPOEpochs(upd, data, EPOCHS, MINIBATCHES, seed=E.SEED), upd


def weights_and_state(upd):
    """E.snapshot without the per-row outputs: what an optimiser step moves"""
    snap = E.snapshot(upd)
    return {k: snap[k] for k in ('policy', 'value', 'm0', 'v0', 'm1', 'v1', 'state')}
