"""CPU: every kernel of the cross-compiled libenvbuild_hip.so is accounted for by tests/_kernel_census.py — an instantiation of the
rollout and closed-loop families is a key of HELD (launched and held against the oracle by tests/test_gpu_kernel_census.py, or
Unreachable with the reason), every other family's instantiation count is in COUNTED.  A kernel or an instantiation that joins the
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
    assert len(K.HELD) == 141 and sum(K.COUNTED.values()) == 167 and not set(K.COUNTED) & set(K.HELD_FAMILIES)


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
