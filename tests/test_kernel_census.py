"""CPU: every kernel of the cross-compiled libenvbuild_hip.so is accounted for by tests/_kernel_census.py — an instantiation of the
rollout and closed-loop families is a key of HELD (launched and held against the oracle by tests/test_gpu_kernel_census.py, or
Unreachable with the reason), an instantiation of the one-launch env kernels a key of ENV_HELD (tests/test_gpu_env_census.py; every
one a Case), every other family's instantiation count is in COUNTED.  A kernel or an instantiation that joins the
library makes this fail, naming it, until someone has decided where it belongs."""
import collections
import glob
import os
import re

import numpy as np
import pytest

from env_build_amd import build as eb_build
from env_build_amd.endtoend_env_utils import VEH_NUM
from tests import _kernel_census as K
from tests._helpers import ROOT

FAMILY_COUNTS = {'rollout_fused_4x8': 24, 'rollout_fused_4x4': 12, 'rollout_fused_1x4': 12, 'rollout_tape_4x8': 6, 'rollout_tape_4x4': 12,
                 'rollout_tape_1x4': 12, 'rollout_gated_4x8': 12, 'rollout_gated_4x4': 12, 'rollout_gated_1x4': 12,
                 'policy_rollout_kernel': 9, 'policy_rollout_grad_kernel': 9, 'policy_rollout_sample_kernel': 9}


@pytest.fixture(scope='module')
def kernels():
    return K.library_kernels(eb_build.build())


def test_every_kernel_of_the_library_is_held_or_counted(kernels):
    assert len(kernels) == 308 and len({k.symbol for k in kernels}) == 308
    extra, missing, counts = K.census(kernels)
    assert not extra, 'kernels of the held families that are no row of HELD: %s' % extra
    assert not missing, 'rows of HELD the library has no kernel for: %s' % [K.row_id(k) for k in missing]
    assert not counts, 'families whose instantiation count (found, COUNTED) changed or that COUNTED does not know: %s' % counts
    found = collections.Counter(k.family for k in kernels)
    assert {f: found[f] for f in K.HELD_FAMILIES} == FAMILY_COUNTS
    assert found['env_step_kernel'] == 45 and found['env_reset_pool_kernel'] == 15
    assert len(K.HELD) == 141 and len(K.ENV_HELD) == 60 and sum(K.COUNTED.values()) == 107
    assert not set(K.COUNTED) & set(K.ALL_HELD_FAMILIES) and not set(K.HELD) & set(K.ENV_HELD)
    assert len(K.HELD) + len(K.ENV_HELD) + sum(K.COUNTED.values()) == 308


def test_rows_are_cases_or_unreachable_with_a_reason():
    kinds = collections.Counter(type(r).__name__ for r in K.HELD.values())
    assert kinds == {'Case': 123, 'Unreachable': 18}, dict(kinds)
    for key, r in K.HELD.items():
        if isinstance(r, K.Case):
            assert K.claimed_kernel(r) == key, (key, r)          # the row's arguments reach the row's kernel by the host's rules
            assert r.task == K.TASKS[key[1]] and r.mode == 'training'
            if r.units is not None:
                assert r.n_veh == VEH_NUM[r.task] and K.batch_of(r) == 65
            else:
                ept = K.envs_per_tile(r.tile, r.n_veh)
                assert K.batch_of(r) == 2 * ept + 3 and r.n_veh == (16 if key[2] else 5 if r.task == 'right' else 9)
        else:
            assert isinstance(r, (K.Unreachable, K.Faulted)) and r.reason.strip(), key
            if isinstance(r, K.Unreachable):                     # allowed for the binary16 gated kernels only
                assert key[0] in K.GATED and key[-1] == 'f16' and 'eb_rollout_gated' in r.reason and 'storage_f16' in r.reason, key
    assert len(K.reachable()) == 123 and len({K.row_id(k) for k in K.HELD}) == 141
    assert K.batch_of(K.HELD[('rollout_fused_4x8', 0, True, 8, 'f32')]) == 131
    assert K.batch_of(K.HELD[('rollout_fused_1x4', 0, True, 4, 'f32')]) == 35
    assert K.batch_of(K.HELD[('rollout_tape_1x4', 2, False, 'f32')]) == 105


def test_env_rows_are_cases_and_claim_their_key():
    """ENV_HELD: 3 tasks x 5 (tile, waves) shapes x 4 kinds = 60 keys, every one a Case whose forced tile and waves reach the key by
    the host's rule (launch_env_step); the feature rows sit on the 15 plain-step and the 15 auto-reset kernels"""
    assert len(K.ENV_HELD) == 60 and all(isinstance(r, K.Case) for r in K.ENV_HELD.values())
    want = {K.env_key(kind, t, et, nw) for kind in K.ENV_KINDS for t in range(3) for et, nw in K.ENV_SHAPES}
    assert set(K.ENV_HELD) == want and len(want) == 60
    assert collections.Counter(k[0] for k in K.ENV_HELD) == {'env_step_kernel': 45, 'env_reset_pool_kernel': 15}
    for key, r in K.ENV_HELD.items():
        assert K.claimed_env_kernel(r) == key, (key, r)
        assert r.task == K.TASKS[key[1]] and r.n_veh == VEH_NUM[r.task] and r.mode == 'training' and r.waves == key[-1]
        assert K.env_batch_of(r) == 2 * key[2] + 3 and r.entry == K.ENV_ENTRY[K.env_kind(r)]
        if key[0] == 'env_step_kernel':
            assert (key[3], key[4]) == {'step': (False, False), 'auto': (False, True), 'obs': (True, False)}[K.env_kind(r)]
        else:
            assert K.env_kind(r) == 'reset'
    assert len(K.ENV_NEW) == 24 and all(k[-1] == 4 and k[2] in (16, 32) for k in K.ENV_NEW)
    assert collections.Counter(f for f, _ in K.ENV_FEATURES) == {'flow': 15, 'flow_auto': 15, 'time_limit': 15}
    for f, k in K.ENV_FEATURES:
        assert k in K.ENV_HELD and k[0] == 'env_step_kernel' and not k[3] and k[4] == (f != 'flow')
    rows = K.env_rows()
    assert len(rows) == 105 and len({r[0] for r in rows}) == 105
    # the default rule: waves left at 0, eight waves per block while the grid has at most 3 blocks per CU, on the small tiles only
    free = lambda tile: K.ENV_HELD[K.env_key('step', 0, 64, 4)]._replace(tile=tile, waves=0)
    assert K.claimed_env_kernel(free(2), n_env=16 * 768, n_cu=256) == K.env_key('step', 0, 16, 8)
    assert K.claimed_env_kernel(free(2), n_env=16 * 768 + 1, n_cu=256) == K.env_key('step', 0, 16, 4)
    assert K.claimed_env_kernel(free(1), n_env=32 * 768, n_cu=256) == K.env_key('step', 0, 32, 8)
    assert K.claimed_env_kernel(free(1), n_env=32 * 768 + 1, n_cu=256) == K.env_key('step', 0, 32, 4)
    assert K.claimed_env_kernel(free(1), n_env=32 * 3 * 213 + 1, n_cu=213) == K.env_key('step', 0, 32, 4)
    assert K.claimed_env_kernel(free(0), n_env=64, n_cu=256) == K.env_key('step', 0, 64, 4)
    assert K.claimed_env_kernel(free(0)._replace(waves=8)) == K.env_key('step', 0, 64, 4)      # no eight-wave kernel on 64-env tiles


def test_the_env_witness_rejects_the_eight_wave_twin_and_a_new_tile_is_unaccounted_for(kernels):
    for key in K.ENV_NEW:
        twin = key[:-1] + (8,)
        assert twin in K.ENV_HELD
        K.check_witness(key, [key])
        with pytest.raises(AssertionError, match='claims %s' % K.row_id(key)):
            K.check_witness(key, [twin])
    key = K.env_key('auto', 1, 16, 4)
    with pytest.raises(AssertionError, match='also launches'):                        # (the reset as a launch of its own)
        K.check_witness(key, [key, K.env_key('reset', 1, 16, 4)])
    with pytest.raises(AssertionError, match='claims env_step_kernel-1-16-0-1-4'):    # the plain step where the auto reset is claimed
        K.check_witness(key, [K.env_key('step', 1, 16, 4)])
    p = K.parse
    assert p('_ZN2eb15env_step_kernelILi2ELi32ELb1ELb0ELi8EEEvNS_11EnvStepArgsE')[:2] == ('env_step_kernel', (2, 32, True, False, 8))
    assert p('_ZN2eb21env_reset_pool_kernelILi0ELi64ELi4EEEvNS_11EnvStepArgsE')[:2] == ('env_reset_pool_kernel', (0, 64, 4))
    with open(eb_build.LIB, 'rb') as fh:
        data = fh.read()
    for new in ('_ZN2eb15env_step_kernelILi0ELi128ELb0ELb0ELi4EEEvNS_11EnvStepArgsE',       # a 128-env tile
                '_ZN2eb15env_step_kernelILi0ELi64ELb0ELb0ELi8EEEvNS_11EnvStepArgsE',        # eight waves on the 64-env tile
                '_ZN2eb21env_reset_pool_kernelILi1ELi16ELi2EEEvNS_11EnvStepArgsE'):         # two waves per block
        extra, missing, counts = K.census([K.parse(s) for s in K.kernel_symbols(data + new.encode() + b'.kd\0')])
        assert extra == [new] and not missing and not counts
    gone = K.env_key('obs', 2, 16, 4)
    extra, missing, counts = K.census([k for k in kernels if K.key_of(k) != gone])
    assert missing == [gone] and not extra and not counts


def test_no_header_declares_a_gated_fp16_entry():
    """what makes the 18 rollout_gated_*<..., _Float16> rows Unreachable: eb_rollout_gated takes fp32 rows and is the only gated entry.
    If a binary16 gated entry appears, those rows must become Cases."""
    declared = set()
    for path in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        with open(path) as fh:
            text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', fh.read(), flags=re.S)
        declared |= set(re.findall(r'\b(eb_\w+)\s*\(', text))
    assert 'eb_rollout_gated' in declared and 'eb_rollout_step_f16' in declared and 'eb_rollout_tape_f16' in declared
    gated = {d for d in declared if re.search(r'_gate(d|_|$)', d)}
    assert gated == {'eb_rollout_gated', 'eb_rollout_gated_blocks', 'eb_gate_feed'}, sorted(gated)
    assert not {d for d in gated if '16' in d}


def test_the_parser_sees_template_arguments_and_a_new_kernel_is_unaccounted_for(kernels):
    by_family = {}
    for k in kernels:
        by_family.setdefault(k.family, k)
    for family in K.HELD_FAMILIES:                               # one name per held family: task, then the family's other axes
        k = by_family[family]
        assert k.args is not None and K.key_of(k) in K.HELD and k.args[0] in (0, 1, 2), k
    p = K.parse
    assert p('_ZN2eb17rollout_fused_4x8ILi2ELb1ELi3EDF16_EEvPKT2_PS1_iiiijiPdPKhNS_9FusedArgsE')[:2] == ('rollout_fused_4x8', (2, True, 3, 'f16'))
    assert p('_ZN2eb17rollout_fused_4x4ILi0ELb0ELi4EfEEvPKT2_PS1_iiiijiPdPKhNS_9FusedArgsE')[:2] == ('rollout_fused_4x4', (0, False, 4, 'f32'))
    assert p('_ZN2eb16rollout_tape_1x4ILi1ELb0EfEEvPKT1_PS1_iiiijiNS_9FusedArgsE')[:2] == ('rollout_tape_1x4', (1, False, 'f32'))
    assert p('_ZN2eb17rollout_gated_4x4ILi1ELb1EDF16_EEvPKT1_PS1_iiiijiNS_9FusedArgsE')[:2] == ('rollout_gated_4x4', (1, True, 'f16'))
    assert p('_ZN2eb12_GLOBAL__N_126policy_rollout_grad_kernelILi2ELi2ELi1EEEvNS_21PolicyRolloutGradArgsE')[:2] == (
        'policy_rollout_grad_kernel', (2, 2, 1))
    assert p('_ZN2eb16gate_feed_kernelEijmPKDv4_jPS0_PjPKjS4_i')[:2] == ('gate_feed_kernel', ())
    with pytest.raises(ValueError):
        p('_Z6kernelv')
    # a synthetic extra descriptor name: a ninth record per lane on the 4x8 tile (PF = 9), a fourth task, a new family
    with open(eb_build.LIB, 'rb') as fh:
        data = fh.read()
    for new in ('_ZN2eb17rollout_fused_4x8ILi0ELb1ELi9EfEEvPKT2_PS1_iiiijiPdPKhNS_9FusedArgsE',
                '_ZN2eb12_GLOBAL__N_121policy_rollout_kernelILi3ELi2ELi2EEEvNS_17PolicyRolloutArgsE'):
        extra, missing, counts = K.census([K.parse(s) for s in K.kernel_symbols(data + new.encode() + b'.kd\0')])
        assert extra == [new] and not missing and not counts
    extra, missing, counts = K.census([K.parse(s) for s in K.kernel_symbols(data + b'_ZN2eb10new_kernelILi0EEEvPf.kd\0')])
    assert not extra and not missing and counts == {'new_kernel': (1, 0)}
    extra, missing, counts = K.census([K.parse(s) for s in K.kernel_symbols(data + b'_ZN2eb10gae_kernelILi1EEEvPf.kd\0')])
    assert counts == {'gae_kernel': (2, 1)}
    extra, missing, counts = K.census([k for k in kernels if K.key_of(k) != ('rollout_tape_4x8', 1, True, 'f16')])
    assert missing == [('rollout_tape_4x8', 1, True, 'f16')] and not extra and not counts


def test_the_witness_comparison_rejects_a_twin():
    key = ('rollout_gated_4x8', 1, False, 'f32')
    K.check_witness(key, [key])
    with pytest.raises(AssertionError, match='claims rollout_gated_4x8-1-0-f32'):       # the FAST twin of what the row claims was launched
        K.check_witness(key, [('rollout_gated_4x8', 1, True, 'f32')])
    with pytest.raises(AssertionError, match='also launches'):
        K.check_witness(key, [key, ('rollout_fused_4x4', 1, False, 4, 'f32')])
    with pytest.raises(AssertionError, match='no held kernel'):
        K.check_witness(key, [])
    # the rules behind a claim: the slot count decides FAST per tile, rolling loads exist on the 4x8 tile only, a 4x8 tape that is not
    # FAST runs on the 4x4 tile
    r = K.rollout_kernel
    assert r('fused', 'left', 16, 0, 1, 'f32') == ('rollout_fused_4x8', 0, True, 3, 'f32')
    assert r('fused', 'left', 9, 0, 0, 'f16') == ('rollout_fused_4x8', 0, False, 8, 'f16')
    assert r('fused', 'right', 16, 1, 1, 'f32') == ('rollout_fused_4x4', 2, True, 4, 'f32')
    assert r('fused', 'left', 128, 2, 0, 'f32') == ('rollout_fused_1x4', 0, False, 4, 'f32')    # 128 divides 256 lanes, not 64
    assert r('tape', 'straight', 9, 0, 0, 'f32') == ('rollout_tape_4x4', 1, False, 'f32')
    assert r('gated', 'straight', 9, 0, 0, 'f32') == ('rollout_gated_4x8', 1, False, 'f32')
    case = K.HELD[('rollout_fused_4x8', 0, True, 3, 'f32')]
    assert K.plan_kernel(case, (0, 3, 1, 1)) == ('rollout_fused_4x8', 0, True, 3, 'f32')
    assert K.plan_kernel(case, (0, 3, 0, 1)) == ('rollout_fused_4x8', 0, True, 8, 'f32')


def test_host_handles_of_every_kernel_are_in_the_symbol_table(kernels):
    """the GPU witness resolves a graph node's `func` through these: every kernel's handle is an OBJECT symbol of the unstripped library
    under the kernel's own mangled name, the closed-loop ones (anonymous namespace) as local symbols"""
    with open(eb_build.LIB, 'rb') as fh:
        table = K.elf_symbols(fh.read())
    held = [k for k in kernels if k.family in K.HELD_FAMILIES]
    assert len(held) == 141 and all(k.symbol in table for k in held)
    assert len({table[k.symbol] for k in held}) == 141
    env = [k for k in kernels if k.family in K.ENV_FAMILIES]
    assert len(env) == 60 and all(k.symbol in table for k in env)
    assert len({table[k.symbol] for k in held + env}) == 201


def test_every_row_has_a_vehicle_near_an_ego_in_its_first_tile():
    """the scenes of the GPU rows (seeded, so decided here): some vehicle within 3.5 m of its ego among the first tile's envs — the
    penalty queue of the first block is not empty"""
    seen = set()
    for key, case in K.reachable():
        if case.units is not None or (case.task, case.n_veh, K.batch_of(case)) in seen:
            continue
        seen.add((case.task, case.n_veh, K.batch_of(case)))
        inp = K.scene_inputs(case)
        ept = (K.batch_of(case) - 3) // 2
        veh = inp['veh'].reshape(len(inp['ego']), case.n_veh, 4)[:ept]
        d = np.hypot(veh[:, :, 0] - inp['ego'][:ept, 3:4], veh[:, :, 1] - inp['ego'][:ept, 4:5])
        assert (d < 3.5).any(), (key, float(d.min()))
