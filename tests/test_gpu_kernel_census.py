"""-m gpu: every reachable row of tests/_kernel_census.HELD — one per instantiation of the rollout and closed-loop kernel families, 123
rows — launches the kernel it claims and that launch is right.

Numerics, by the suite's existing bars: fused and tape rows against the oracle as test_every_tile_shape_computes_the_same_bits does
(observations bit for bit, out5 bit for bit against the oracle in the kernels' summation order; binary16 rows through rollout_step_f16 / rollout_tape_f16 on both sides); gated rows
with every gate opened in advance, by test_gated_rollout_with_open_gates_equals_stepwise's assertions (status word [0, 0] included);
closed-loop rows through the functions the closed-loop tests themselves call (tests/_policy.py, _policy_rollout_grad.py,
_policy_rollout_sample.py) at 65 rows, two steps, the task's native slot count, one hidden layer of the row's width.

Witness: the row's entry is captured on a side stream (nothing runs), and every kernel node's host-side handle is resolved to a kernel
of libenvbuild_hip.so (tests/_kernel_census.handle_names).  The row's kernel must be among the nodes and no other kernel of the held
families may be.  Should a runtime hand out something else than the handle, the rollout rows fall back to eb_debug_rollout_plan with the
restated launch rules (_kernel_census.plan_kernel); WITNESS records what each family got.

Shapes: two full tiles plus three envs (a second block and a ragged tail), three steps, 16 slots for FAST rows and 9 (5 on `right`) for
the others, each task tiled in place.  Handles, oracle models and scenes are shared per (task, slot count).  Wall time of the module on
an MI355X: 3.6 s for the 123 rows (the slowest, the first to create a handle pair, 0.45 s; the first row of each task 0.2 s; every other row ≈ 10 ms).

A faulted card gets no more launches: a row that ends in a HIP error makes every later row skip; a failing comparison does not."""
import ctypes as C

import numpy as np
import pytest

from env_build_amd import _capi
from tests import _capture, _kernel_census as K, _policy, _policy_rollout_grad as PG, _policy_rollout_sample as PS
from tests._helpers import (DeviceModel, HostModel, check_out5 as _check_out5, check_out5_steps as _check_gated, initial_obs as _initial_obs,
                            oracle_lib, record_host, stepwise as _stepwise)

pytestmark = pytest.mark.gpu
STEPS = 3
ROWS = K.reachable()
WITNESS = {}                 # family -> 'graph' / 'plan': the witness its rows got
_faulted = []                # the rows that ended in a HIP error
_models, _scenes, _handles = {}, {}, {}


_is_hip_error = K.is_hip_error


def _pair(case):
    key = (case.task, case.n_veh, case.mode)
    if key not in _models:
        _models[key] = (record_host(case.task, n_veh=case.n_veh, mode=case.mode),
                        DeviceModel(case.task, n_veh=case.n_veh, mode=case.mode))
    return _models[key]


def _scene(case, host):
    key = (case.task, case.n_veh, K.batch_of(case))
    if key not in _scenes:
        inp = K.scene_inputs(case, STEPS)
        _scenes[key] = (inp, _initial_obs(host, inp))
    return _scenes[key]


def _kernel_handles(dev):
    if not _handles:
        _handles.update(K.handle_names(_capi.HIP_LIB_PATH, dev.api.lib))
    return _handles


def _launched(dev, call, what):
    """the held-family kernels `call(stream)` enqueues, from a capture of it -> set of keys, or None when a node's func is no handle of
    the library (the graph witness is not available on this runtime)"""
    dev.torch.cuda.synchronize()
    g = _capture.capture(_capture.side_stream(), lambda raw: call(C.c_void_p(raw)), what)
    try:
        funcs = K.kernel_node_funcs(g)
    finally:
        g.close()
    assert funcs, '%s: the capture holds no kernel node' % what
    table = _kernel_handles(dev)
    if any(f not in table for f in funcs):
        return None
    return {K.key_of(table[f]) for f in funcs if table[f].family in K.HELD_FAMILIES}


# ---- rollout rows ----
def _rollout_call(dev, case, inp, obs0):
    """the row's entry as one C call over device arrays -> call(stream)"""
    t, p, B = dev.torch, dev._ptr, len(obs0)
    ob = dev._in(obs0.astype(np.float16).view(np.int16), np.int16) if case.storage == 'f16' else dev._in(obs0)
    ac, ri = dev._in(inp['actions']), dev._in(inp['ref_idx'], np.int32)
    out, work = t.empty_like(ob), t.empty_like(ob)
    kind = K.KIND_OF_ENTRY[case.entry]
    fn = getattr(dev.api, case.entry)
    if kind == 'fused':
        out5, sc = dev._out((5, B)), dev._out((B, 2))
        return lambda s, keep=(ob, ac, ri, out, out5, sc): fn(dev.h, B, p(ob), p(ac[0]), p(ri), 0, p(out), p(out5), p(sc), s)
    out5 = dev._out((STEPS, 5, B))
    if kind == 'tape':
        return lambda s, keep=(ob, ac, ri, work, out, out5): fn(dev.h, B, STEPS, p(ob), p(ac), p(ri), 0, p(work), p(out), p(out5), s)
    nb = dev.gated_blocks(B)
    assert nb >= 1
    steps, ready = dev._out((STEPS,) + tuple(ob.shape)), dev._in(np.ones(STEPS, np.int32), np.int32)
    done, status = dev._in(np.zeros((STEPS, nb, 16), np.int32), np.int32), dev._in(np.zeros(2, np.int32), np.int32)
    return lambda s, keep=(ob, ac, ri, work, out, out5, steps, ready, done, status): fn(
        dev.h, B, STEPS, p(ob), p(ac), p(ri), 0, p(work), p(out), p(out5), p(steps), p(ready), p(done), nb, p(status), 1 << 22, s)


def _rollout_numerics(host, dev, case, inp, obs0):
    kind, f16 = K.KIND_OF_ENTRY[case.entry], case.storage == 'f16'
    ri, B = inp['ref_idx'], len(obs0)
    first = obs0.astype(np.float16).view(np.uint16) if f16 else obs0
    if kind == 'fused':
        step = (lambda m, o, a: m.rollout_step_f16(o, a, ri)) if f16 else (lambda m, o, a: m.rollout_step(o, a, ri))
        obs_h = obs_d = first
        for t in range(STEPS):
            obs_h, o5_h, sc_h = step(host, obs_h, inp['actions'][t])
            obs_d, o5_d, sc_d = step(dev, obs_d, inp['actions'][t])
            assert np.array_equal(obs_d, obs_h), 'step %d: %d of %d words differ' % (t, int((obs_d != obs_h).sum()), obs_h.size)
            assert np.array_equal(sc_d, sc_h)
            _check_out5(o5_d, o5_h, 'step %d' % t, exact=True)
        if not f16:                                              # the no-reward form of the kernel (fp32 rows only have the entry)
            nxt = dev.compute_next_obses(obs_d, inp['actions'][0] * 0.3, ri)
            assert np.array_equal(nxt, host.compute_next_obses(obs_h, inp['actions'][0] * 0.3, ri))
    elif kind == 'tape':
        tape = (lambda m: m.rollout_tape_f16(first, inp['actions'], ri)) if f16 else (lambda m: m.rollout_tape(first, inp['actions'], ri))
        out_d, o5_d = tape(dev)
        out_h, o5_h = tape(host)
        assert np.array_equal(out_d, out_h), '%d of %d words differ' % (int((out_d != out_h).sum()), out_h.size)
        for t in range(STEPS):
            _check_out5(o5_d[t], o5_h[t], 'step %d' % t, exact=True)
    else:
        want_obs, want_o5, want_states = _stepwise(host, obs0, inp, STEPS)
        nb = dev.gated_blocks(B)
        assert nb >= 1
        for publish in (True, False):
            out, o5, steps, done, status = dev.rollout_gated(obs0, inp['actions'], ri, publish_obs=publish)
            assert status.tolist() == [0, 0] and done.shape == (STEPS, nb, 16) and done.all()
            assert np.array_equal(out, want_obs)
            _check_gated(o5, want_o5, exact=True)
            if publish:
                assert np.array_equal(steps, want_states)


def _rollout_row(key, case):
    host, dev = _pair(case)
    inp, obs0 = _scene(case, host)
    B = K.batch_of(case)
    dev.set_tile(case.tile)
    dev.set_rollout_sched(case.rolling, -1)
    try:
        assert len(obs0) == B and dev.rollout_plan(B)[0] == case.tile
        _rollout_numerics(host, dev, case, inp, obs0)
        try:
            launched = _launched(dev, _rollout_call(dev, case, inp, obs0), case.entry)
        except _capture.CaptureError:
            if case.entry != 'rollout_gated':                    # (the capture census leaves the gated entry out: it may refuse)
                raise
            launched = None
        if launched is None:
            launched, how = {K.plan_kernel(case, dev.rollout_plan(B))}, 'plan'
        else:
            how = 'graph'
        dev.torch.cuda.synchronize()
        WITNESS.setdefault(key[0], how)
        assert WITNESS[key[0]] == how
        K.check_witness(key, launched)
    finally:
        dev.set_tile(-1)
        dev.set_rollout_sched(-1, -1)


# ---- closed-loop rows ----
def _policy_call(dev, m, case, obs0, ref_idx, steps=2):
    """the closed-loop entry as one C call over device arrays, every output wanted -> call(stream)"""
    t, p = dev.torch, dev._ptr
    ob, ri = dev._in(obs0), dev._in(ref_idx, np.int32)
    n, D = ob.shape
    if case.entry == 'policy_rollout':
        last, out5, act, obs = dev._out((n, D)), dev._out((steps, 5, n)), dev._out((steps, n, 2)), dev._out((steps, n, D))
        punish, safe = dev._out((n,)), dev._out((n,), np.uint8)
        return lambda s, keep=(ob, ri, last, out5, act, obs, punish, safe): dev.api.policy_rollout(
            dev.h, m, n, steps, p(ob), p(ri), 0, C.c_float(1.0), 0, p(last), p(out5), p(act), p(obs), p(punish), p(safe), s)
    H = PG if case.entry == 'policy_rollout_grad' else PS
    count = H.param_count(dev, m)
    bufs = {k: t.empty(s, device=dev.dev) for k, s in H.shapes(n, D, steps, count).items()}
    if H is PG:
        need = PG.workspace_bytes(dev, m, n, steps)
        ws = t.empty((max(need, 16),), dtype=t.uint8, device=dev.dev)
        return lambda s, keep=(ob, ri, ws, bufs): dev.api.policy_rollout_grad(
            dev.h, m, n, steps, p(ob), p(ri), 0, C.c_float(1.0), PG.floats(PG.W5), p(ws), need, *[p(bufs[k]) for k in PG.OUTPUTS], s)
    need = PS.workspace_bytes(dev, m, n, steps, 1)
    ws = t.empty((max(need, 16),), dtype=t.uint8, device=dev.dev)
    fields = dict(n_env=n, steps=steps, action_range=1.0, w_logp=0.0, w5=PS.W5, seed=PS.SEED, counter=0, obs_in=PS.raw(ob), ref_idx=PS.raw(ri),
                  workspace=PS.raw(ws) if need else None, workspace_bytes=need, **{PS.FIELD[k]: PS.raw(v) for k, v in bufs.items()})
    return lambda s, keep=(ob, ri, ws, bufs): PS.call(dev, m, stream=s, **fields)


def _policy_row(key, case):
    task, N, units = case.task, case.n_veh, case.units
    if case.entry == 'policy_rollout':
        _policy.every_output_equals_the_loop((task, N, units, 1), sizes=(65,), loop_steps=2, horizons=((2, 0), (1, 1)), short=2, others=False)
        obs0, ref_idx, net, scale = _policy.scene(task, N, units, 1)
        dev = DeviceModel(task, n_veh=N)
        m = _policy.f16_mlp(dev, *net, scale)
    else:
        if case.entry == 'policy_rollout_grad':
            PG.forward_and_reverse_equal_the_loop((task, N, units, 1, 'elu'), sizes=(65,), horizons=(2,), only_g_params_at=2, others=False)
        else:
            PS.forward_equals_the_loop((task, N, units, 1, 'elu'), sizes=(65,), horizons=(2,), others=False)
            PS.reverse_equals_the_loop((task, N, units, 1, 'elu'), sizes=(65,), horizons=(2,))
        obs0, ref_idx, net, scale = PG.scene(task, N, units, 1, hact='elu')
        dev = PG.model(task, N)
        m = dev.make_mlp(*net, scale)
    try:
        launched = _launched(dev, _policy_call(dev, m, case, obs0[:65], ref_idx[:65]), case.entry)
        dev.torch.cuda.synchronize()
        assert launched is not None, 'a kernel node of %s resolves to no handle of the library: no witness for the closed-loop rows' % case.entry
        WITNESS.setdefault(key[0], 'graph')
        K.check_witness(key, launched)
    finally:
        dev.api.mlp_destroy(m)


@pytest.mark.parametrize('key,case', ROWS, ids=[K.row_id(k) for k, _ in ROWS])
def test_the_row_launches_its_kernel_and_the_launch_is_right(key, case):
    if _faulted:
        pytest.skip('an earlier census row faulted')
    try:
        (_policy_row if case.units is not None else _rollout_row)(key, case)
    except BaseException as e:                                   # noqa: BLE001  (re-raised; a HIP error ends the module's launches)
        if _is_hip_error(e):
            _faulted.append(K.row_id(key))
        raise


def test_a_hip_error_is_told_from_a_failing_comparison():
    assert _is_hip_error(_capi.EbError('envbuild(hip) error -3: hipLaunchKernel: an illegal memory access was encountered (hipError 700)'))
    assert _is_hip_error(RuntimeError('HIP error: an illegal memory access was encountered'))
    assert not _is_hip_error(AssertionError('HIP error in the text of a comparison')) and not _is_hip_error(ValueError('bad argument'))
    assert not _is_hip_error(_capi.EbError('envbuild(hip) error -4: eb_mlp_set_layer has not been called for every layer'))
    print('witness per family: %s; faulted rows: %s' % (sorted(WITNESS.items()), _faulted))
