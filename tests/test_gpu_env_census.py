"""-m gpu: every row of tests/_kernel_census.ENV_HELD — one per instantiation of the one-launch env kernels env_step_kernel<TASK, ET,
OBS, AUTO, NW> and env_reset_pool_kernel<TASK, ET, NW>, 60 rows — and the 45 feature rows of ENV_FEATURES launch the kernel they claim,
and that launch is right.  The tile AND the waves per block are forced (eb_debug_set_tile, eb_debug_set_env_waves): left to the grid,
a small-tile launch takes four waves only above 3 * n_cu blocks, which no other test of the suite reaches — 24 of the 60 kernels (16- and
32-env tiles x four waves) are launched by these rows alone, among them the only code with FUSED_FLOW, DRAW_LATE and EVEN
(csrc/eb_env_step_body.h).

Numerics, by the suite's existing bars (tests/test_gpu_parity.py): the case functions of tests/_env_step_check.py on DeviceModel with
tile and waves forced (each asserts the one launch against the HIP library's single calls, bit for bit) and on the oracle; the two results
bit for bit, the penalty sums and the 16-row dictionary bit for bit too (the oracle sums them in the kernels' order).  step: composite_case; auto reset:
auto_reset_case; observation: eb_get_obs against the oracle and masked_obs_case; masked reset: reset_pool_case; features: flow_rule_case
(plain step) and flow_auto_reset_case, time_limit_case (auto reset) at K = 2 routes per approach.  The oracle's result is computed once
per scene (a kind, a task, a batch) and shared by the rows of every tile shape.

Witness: the row's entry — the makers of tests/_capture_cases.py — captured on a side stream with the same tile and waves (nothing
runs); every kernel node's handle is resolved to a kernel of libenvbuild_hip.so (tests/_kernel_census.handle_names).  The row's kernel
must be among the nodes and no other kernel of the two families may be.  There is no fallback witness: a node that resolves to no handle
fails the row.  The default rule (waves left to the grid) is held by witness alone at 3 * n_cu blocks and one env more.

Shapes: two full tiles plus three envs (35 / 67 / 131), native slot counts, 14 candidates (24 for the flow rows), 6 flow steps, 2 with
auto reset — tests/test_env_census_scenes.py holds on the CPU that these scenes emit, finish and mask what the rows are about.
Wall time of the module on an MI355X: 2.4 s for the 105 rows and the two default-rule cases — tests/test_gpu_kernel_census.py takes 3.6 s
for its 123 — (the slowest, the first to create a handle pair, 0.5 s; the first row of each task 0.2 s; a default-rule case 0.1 s; every
other row 10 - 20 ms); the last test prints it.

A faulted card gets no more launches: a row that ends in a HIP error makes every later row skip; a failing comparison does not."""
import time

import numpy as np
import pytest

from env_build_amd import _capi
from tests import _capture, _capture_cases as CC, _env_census as EC, _kernel_census as K
from tests._helpers import DeviceModel, HostModel, bits_equal, check_out5, oracle_lib, record_host

pytestmark = pytest.mark.gpu
ROWS = K.env_rows()
WITNESS = {}                 # family -> 'graph'
FIRST = {}                   # key of a kernel of K.ENV_NEW -> how its first launch compared with the oracle
_faulted = []                # the rows that ended in a HIP error
_want, _handles, _clock = {}, {}, []


def _on_cpu(t, **kw):
    return record_host(t, **kw)


def _reference(kind, task, B):
    if (kind, task, B) not in _want:
        _want[(kind, task, B)] = EC.run_row(kind, _on_cpu, task, B)
    return _want[(kind, task, B)]


def _compare(want, got, B, what, nan_ok):
    """test_gpu_parity's comparison of two results of a case function, over nested lists (traces, the masked reset's four results)"""
    if isinstance(want, (list, tuple)):
        assert len(want) == len(got), what
        for k, (w, g) in enumerate(zip(want, got)):
            _compare(w, g, B, '%s[%d]' % (what, k), nan_ok)
    elif want is None:
        assert got is None, what
    elif want.dtype == np.float32 and want.shape == (5, B):
        check_out5(got, want, what, exact=True)
    elif want.shape == (16, B):
        bits_equal(got, want, what)
    else:
        assert np.array_equal(want, got, equal_nan=nan_ok), '%s: %d of %d elements differ' % (what, int((want != got).sum()), want.size)


def _launched(call, tile, waves, what):
    """the kernels of the two env families `call.run(stream)` enqueues with the tile and the waves set as given, from a capture of it"""
    dev = call.dev
    dev.set_tile(tile)
    dev.set_env_waves(waves)
    try:
        dev.torch.cuda.synchronize()
        g = _capture.capture(_capture.side_stream(), call.run, what)
        try:
            funcs = K.kernel_node_funcs(g)
        finally:
            g.close()
        dev.torch.cuda.synchronize()
    finally:
        dev.set_tile(-1)
        dev.set_env_waves(0)
    if not _handles:
        _handles.update(K.handle_names(_capi.HIP_LIB_PATH, dev.api.lib))
    assert funcs, '%s: the capture holds no kernel node' % what
    assert all(f in _handles for f in funcs), '%s: a kernel node resolves to no handle of the library: no witness' % what
    return [K.key_of(_handles[f]) for f in funcs if _handles[f].family in K.ENV_FAMILIES]


def _witness_call(kind, task, B):
    size = {'n': B}
    if kind == 'obs':
        return CC._get_obs(size, 'A', task)
    if kind == 'reset':
        return CC._env_reset_pool(size, 'A', task, M=K.ENV_CAND)
    if kind in ('flow', 'flow_auto'):
        return CC._env_step_auto_reset_flow(size, 'A', task, auto_reset=kind == 'flow_auto')
    return CC._env_step(size, 'A', task, auto_reset=kind != 'step', time_limit=kind == 'time_limit')


def _numerics(kind, case, B):
    task, made = case.task, []

    def on_gpu(t, **kw):
        d = DeviceModel(t, **kw)
        made.append(d)
        return d
    try:
        if kind == 'obs':
            from tests._env_step_check import masked_obs_case
            ego, cand, cmode, light, ref, virtual = EC.obs_scene(task, B)
            dev = on_gpu(task, mode='training')
            dev.set_tile(case.tile)
            dev.set_env_waves(case.waves)
            got = dev.get_obs(ego, cand, cmode, light, ref_idx=ref, virtual=virtual)
            want = _on_cpu(task, mode='training').get_obs(ego, cand, cmode, light, ref_idx=ref, virtual=virtual)
            assert np.array_equal(got, want), '%d of %d words differ' % (int((got != want).sum()), want.size)

            def forced(t, **kw):
                d = on_gpu(t, **kw)
                d.set_tile(case.tile)
                d.set_env_waves(case.waves)
                return d
            if ('masked', task, B) not in _want:
                _want[('masked', task, B)] = masked_obs_case(_on_cpu, task, B=B, M=K.ENV_CAND)
            assert np.array_equal(masked_obs_case(forced, task, B=B, M=K.ENV_CAND), _want[('masked', task, B)])
            return
        want = _reference(kind, task, B)
        got = EC.run_row(kind, on_gpu, task, B, tile=case.tile, waves=case.waves)
        _compare(want, got, B, kind, nan_ok=kind not in ('step', 'reset'))
    finally:
        for d in made:
            d.set_tile(-1)
            d.set_env_waves(0)


def _row(rid, kind, key, case):
    B = K.env_batch_of(case)
    assert K.claimed_env_kernel(case) == key
    try:
        _numerics(kind, case, B)
    except AssertionError:
        if key in K.ENV_NEW:
            FIRST.setdefault(key, 'DIFFERED (%s)' % rid)
        raise
    if key in K.ENV_NEW:
        FIRST.setdefault(key, 'agreed')
    call = _witness_call(kind, case.task, B)
    K.check_witness(key, _launched(call, case.tile, case.waves, rid))
    WITNESS.setdefault(key[0], 'graph')


@pytest.mark.parametrize('rid,kind,key,case', ROWS, ids=[r[0] for r in ROWS])
def test_the_env_row_launches_its_kernel_and_the_launch_is_right(rid, kind, key, case):
    if _faulted:
        pytest.skip('an earlier env census row faulted')
    if not _clock:
        _clock.append(time.perf_counter())
    try:
        _row(rid, kind, key, case)
    except BaseException as e:                                   # noqa: BLE001  (re-raised; a HIP error ends the module's launches)
        if K.is_hip_error(e):
            _faulted.append(rid)
            if key in K.ENV_NEW:
                FIRST.setdefault(key, 'HIP ERROR (%s)' % rid)
        raise


@pytest.mark.parametrize('tile', [2, 1], ids=['16-env-tiles', '32-env-tiles'])
def test_waves_left_to_the_grid_change_at_three_blocks_per_cu(tile):
    """launch_env_step's own rule, by witness alone (nothing executes under capture): eight waves per block up to 3 * n_cu blocks of a
    small tile, four from one env more"""
    if _faulted:
        pytest.skip('an earlier env census row faulted')
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    et = {2: 16, 1: 32}[tile]
    case = K.ENV_HELD[K.env_key('step', 0, 64, 4)]._replace(tile=tile, waves=0)
    try:
        for B, nw in ((et * 3 * n_cu, 8), (et * 3 * n_cu + 1, 4)):
            key = K.claimed_env_kernel(case, n_env=B, n_cu=n_cu)
            assert key == K.env_key('step', 0, et, nw)
            K.check_witness(key, _launched(CC._env_step({'n': B}, 'A', 'left'), tile, 0, 'eb_env_step at %d envs' % B))
    except BaseException as e:                                   # noqa: BLE001
        if K.is_hip_error(e):
            _faulted.append('default rule, tile %d' % tile)
        raise
    print('n_cu %d: %d-env tiles take eight waves up to %d envs, four from %d' % (n_cu, et, et * 3 * n_cu, et * 3 * n_cu + 1))


def test_report():
    """what the rows found (printed; -s shows it): the witness per family, how the first launch of each of the 24 kernels no test launched
    before compared with the oracle, the faulted rows, the module's wall time"""
    took = time.perf_counter() - _clock[0] if _clock else float('nan')
    print('env census: %d rows; witness per family: %s; faulted rows: %s; wall time %.1f s' % (len(ROWS), sorted(WITNESS.items()), _faulted, took))
    for key in K.ENV_NEW:
        print('first launch of %s: %s' % (K.row_id(key), FIRST.get(key, 'not launched')))
    if not _faulted and len(FIRST) == len(K.ENV_NEW):
        assert set(WITNESS) == set(K.ENV_FAMILIES) and set(WITNESS.values()) == {'graph'}
