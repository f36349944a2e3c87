"""GPU (-m gpu): the host checks the five one-launch tape entries share (csrc/eb_capi.hip: check_tape, check_path_arg, cand_path_bits) —
eb_rollout_tape_vjp, eb_rollout_tape_cand, eb_rollout_tape_cand_vjp, eb_rollout_tape_sample, eb_rollout_tape_ilqr.

Per entry, at the smallest shape at which the entries differ (3 envs, 2 steps, the task's native slot count, one candidate / one
sample / no step length): a selecting-mode handle refuses path_id == n_paths, a training-mode handle refuses ref_idx == NULL, and
n_env == 0 returns without touching an output.  Every case ends on the host: nothing here launches a kernel."""
import ctypes as C

import pytest

from tests._tape import NATIVE, TapeModel

pytestmark = pytest.mark.gpu
ENTRIES = ('vjp', 'cand', 'cand_vjp', 'sample', 'ilqr')
TASK, B, H, N_PATHS = 'left', 3, 2, 3
W5 = (C.c_float * 5)(-1.0, 10.0, 0.0, 0.0, 0.0)
SIGMA = (C.c_float * 2)(0.1, 0.1)
FILL_F, FILL_I = 7.5, -7


def outputs(m, entry):
    """the entry's output tensors, in its argument order, filled with a value no launch leaves behind"""
    torch, D, nd = m.torch, m.D, m.D - 4 * m.n_veh
    shapes = dict(vjp=((H, 5, B), (B, D), (B, nd), (H, B, 2)),
                  cand=((1, H, 5, B), (1, B)),
                  cand_vjp=((1, H, 5, B), (1, B), (1, B, nd), (1, H, B, 2)),
                  sample=((1, B), (H, B, 2), (B,), 'i', (H, B, 2), (1, H, B, 2)),
                  ilqr=((1, B), 'i', (B,), (H, B, 2), (H, 6, B), (H, 14, B), (2, B), (1, H, B, 2), (H, 157, B)))[entry]
    return [torch.full((B,), FILL_I, dtype=torch.int32, device=m.dev) if s == 'i' else torch.full(s, FILL_F, device=m.dev) for s in shapes]


def call(m, entry, n_env, obs0, tape, ri, path_id, outs):
    p, o = m._ptr, [m._ptr(t) for t in outs]
    if entry == 'vjp':
        m.api.rollout_tape_vjp(m.h, n_env, H, p(obs0), p(tape), p(ri), path_id, None, 0, None, W5, *o, m.stream)
    elif entry in ('cand', 'cand_vjp'):
        getattr(m.api, 'rollout_tape_' + entry)(m.h, n_env, 1, H, p(obs0), p(tape), p(ri), 0, None, path_id, 0, W5, *o, m.stream)
    elif entry == 'sample':
        m.api.rollout_tape_sample(m.h, n_env, 1, H, p(obs0), p(tape), p(ri), path_id, None, 0, 0, SIGMA, 0.0, 1.0, W5, *o, m.stream)
    else:
        m.api.rollout_tape_ilqr(m.h, n_env, H, 0, p(obs0), p(tape), None, None, p(ri), path_id, None, None, W5, *o, m.stream)


def inputs(m):
    torch = m.torch
    return torch.zeros((B, m.D), device=m.dev), torch.zeros((H, B, 2), device=m.dev), torch.zeros((B,), dtype=torch.int32, device=m.dev)


@pytest.mark.parametrize('entry', ENTRIES)
def test_tape_entry_host_checks(entry):
    sel = TapeModel(TASK, n_veh=NATIVE[TASK], n_future=0, mode='selecting')
    obs0, tape, ri = inputs(sel)
    with pytest.raises(ValueError) as e:                                   # selecting mode: path ids are 0 .. n_paths - 1
        call(sel, entry, B, obs0, tape, None, N_PATHS, outputs(sel, entry))
    assert 'bad path_id' in str(e.value)
    trn = TapeModel(TASK, n_veh=NATIVE[TASK], n_future=0, mode='training')
    with pytest.raises(ValueError) as e:                                   # training mode: the path comes per env
        call(trn, entry, B, obs0, tape, None, 0, outputs(trn, entry))
    assert 'training mode needs ref_idx' in str(e.value)
    for m, r, pid in ((trn, ri, 0), (sel, None, 1)):                       # n_env == 0: a no-op that succeeds
        outs = outputs(m, entry)
        call(m, entry, 0, obs0, tape, r, pid, outs)
        m.torch.cuda.synchronize()
        for k, t in enumerate(outs):
            assert bool((t == (FILL_I if t.dtype == m.torch.int32 else FILL_F)).all()), 'output %d was written' % k
