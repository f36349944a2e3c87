"""CPU (-m "not gpu"): the census of fixture G20 (oracle/gen_golden_env_edges.py) — computed in NumPy from the fixture's INPUTS with
the rule tables of tests/_env_edges.py: every case the replays (tests/_golden_checks.py: check_g20_env_edges; tests/_env_step_check.py:
g20_parked_case) are meant to reach is in the committed files.  It asserts properties of inputs, not of any library: a later edit of
the generator cannot silently drop a case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _env_edges as EE
from tests._helpers import GOLDEN, ROOT, golden

TASKS = ('left', 'straight', 'right')
FILES = [('g20_env_edges_%s' % t, t, None) for t in TASKS] + [('g20w_env_edges_%s_N16' % t, t, 16) for t in TASKS]
IDS = [f[0] for f in FILES]


def load(name):
    z = golden(name)                                                        # allow_pickle=False
    return {k: z[k] for k in z.files}                                       # (decompressed once, not at every g[...] of a loop)


def _counts(task, n_veh):
    return EE.MODE_COUNTS[task] if n_veh is None else EE.tiled_counts(task, n_veh)[1]


def _block_rows(g, i, task, n_veh, mode):
    """the rows of scene i's recorded block that belong to `mode`"""
    block = g['obs'][i, 9:].reshape(-1, 4)
    if n_veh is None:
        slots = [m for m, k in EE.MODE_COUNTS[task].items() for _ in range(k)]
    else:
        slots = EE.tiled_counts(task, n_veh)[0]
    return block[[s for s, m in enumerate(slots) if m == mode]]


@pytest.mark.parametrize('name,task,n_veh', FILES, ids=IDS)
def test_files_are_plain_arrays_of_24_candidates(name, task, n_veh):
    g = load(name)
    n = len(g['label'])
    assert 100 <= n <= 700 and g['label'].dtype.kind == 'U' and g['cand'].shape == (n, 24, 4) and g['cand'].dtype == np.float32
    assert g['obs'].shape == (n, 9 + 4 * sum(_counts(task, n_veh).values()))
    assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) <= 592 * 1024
    if n_veh is not None:
        assert [EE.MODES12[i] for i in g['slot_modes']] == EE.tiled_counts(task, n_veh)[0]
        assert {l[0] for l in g['label']} == set('ABCD')
    else:
        assert {l[0] for l in g['label']} == set(EE.FAMILIES)


@pytest.mark.parametrize('name,task,n_veh', FILES, ids=IDS)
def test_family_a_every_bound_has_an_on_an_inside_and_an_outside_case(name, task, n_veh):
    g = load(name)
    seen, inexact, ud_cases = set(), set(), set()
    for i in range(len(g['label'])):
        ex, ey = g['ego'][i, 3], g['ego'][i, 4]
        for c in np.flatnonzero(g['cand_mode'][i] != EE.VACANT):
            mode = EE.MODES12[g['cand_mode'][i, c]]
            x, y = g['cand'][i, c, 0], g['cand'][i, c, 1]
            alone = int((g['cand_mode'][i] == g['cand_mode'][i, c]).sum()) == 1
            for bname, axis, side, val in EE.filter_bounds(task, mode, ex, ey):
                if not EE.in_range(task, mode, ex, ey, x, y, skip=bname):
                    continue
                inward = np.float32(np.inf if side == '>' else -np.inf)
                coord = (x, y)[axis]
                pos = {float(val): 'on', float(np.nextafter(val, inward)): 'inside', float(np.nextafter(val, -inward)): 'outside'}.get(float(coord))
                if pos is None:
                    continue
                seen.add((mode, bname, pos))
                # every comparison is strict: "on" is out of the recorded block, "inside" is in it
                if alone and mode in _counts(task, n_veh) and EE.stop_line_car(task, mode, ey, g['v_light'][i] or g['virtual'][i]) is None:
                    first = _block_rows(g, i, task, n_veh, mode)[0]
                    assert np.array_equal(first, g['cand'][i, c]) == (pos == 'inside'), g['label'][i]
                want64 = {'y>ey-2': float(ey) - 2, 'x<ex+5': float(ex) + 5, 'x<ex+7': float(ex) + 7}.get(bname)
                if want64 is not None and want64 != float(val):
                    inexact.add((mode, bname))
            if mode == 'ud':             # max(ego_y - 2, -25): either candidate, with ego_y - 2 below / at / above -25
                ey2 = np.float32(ey) - np.float32(2)
                rel = 'below' if ey2 < -25 else 'at' if ey2 == -25 else 'above'
                for which, v in (('ey-2', ey2), ('-25', np.float32(-25))):
                    if y == v:
                        ud_cases.add((rel, which))
    for mode in _counts(task, n_veh):
        for bname, _, _, _ in EE.filter_bounds(task, mode, 0.0, -30.0):
            for pos in ('on', 'inside', 'outside'):
                assert (mode, bname, pos) in seen, (mode, bname, pos)
            if bname in ('y>ey-2', 'x<ex+5', 'x<ex+7'):
                assert (mode, bname) in inexact, (mode, bname)
    if 'ud' in _counts(task, n_veh):
        assert ud_cases == {(r, w) for r in ('below', 'at', 'above') for w in ('ey-2', '-25')}


@pytest.mark.parametrize('name,task,n_veh', FILES, ids=IDS)
def test_family_b_every_mode_has_tie_groups_the_slice_cuts(name, task, n_veh):
    g = load(name)
    counts = _counts(task, n_veh)
    cut_primary, cut_xy, scrambled, late = set(), set(), set(), set()
    for i in range(len(g['label'])):
        ex, ey, lit = g['ego'][i, 3], g['ego'][i, 4], bool(g['v_light'][i] or g['virtual'][i])
        for mode, num in counts.items():
            order = EE.ranked(task, mode, ex, ey, lit, g['cand'][i], g['cand_mode'][i])
            a1 = EE.sort_keys(task, mode)[0][0]
            if len(order) > num:
                last_in, first_out = order[num - 1], order[num]
                if last_in[1 + a1] == first_out[1 + a1]:
                    cut_primary.add(mode)
                    group = [r[0] for r in order if r[1 + a1] == last_in[1 + a1]]
                    if len(group) >= 3 and group != sorted(group) and group != sorted(group, reverse=True):
                        scrambled.add(mode)             # the reference's order of the group is neither the insertion order nor its reverse
                if last_in[1:] == first_out[1:]:
                    cut_xy.add(mode)
            mine = np.flatnonzero(g['cand_mode'][i] == EE.MODES12.index(mode)).tolist()
            if len(mine) >= 6 and len(order) >= num and all(mine.index(r[0]) >= 4 for r in order[:num] if r[0] < 24):
                late.add(mode)                          # the winners are the fifth and later candidates of their mode
    assert cut_primary == set(counts) and cut_xy == set(counts), (cut_primary, cut_xy)
    assert {m for m in counts if len(EE.sort_keys(task, m)) > 1} <= scrambled
    assert late, 'no scene whose winners come after the first four candidates of their mode'
    if n_veh is None:
        assert {m for m, k in counts.items() if k == 2} <= late


REQUIRED = dict(
    C=lambda task, counts: (['C|right|l1v0', 'C|right|l0v1', 'C|right|l2v1'] if task == 'right' else
                            ['C|line|%s|l%dv%d' % (e, a, b) for e in ('on', 'below', 'above') for a, b in ((1, 0), (0, 1), (2, 1), (0, 0))] +
                            ['C|%s|%s' % (k, m) for k in ('tie_y', 'tie_xy', 'last_lost', 'last_won') for m in ('dl', 'du') if m in counts] +
                            ['C|du_x|%s' % k for k in ('outside', 'on', 'on_rounded', 'inside')]),
    D=lambda task, counts: (['D|%s|%s' % (m, k) for m in counts for k in ('0', 'num-1', 'num', 'num+1', 'all24')] +
                            ['D|none', 'D|vacant_odd', 'D|vacant_even', 'D|empty']),
    E=lambda task, counts: (['E|goal|%s|%s' % (b, p) for b in dict(left=('x<-35', 'y>0', 'y<11.25'), straight=('y>35', 'x>0', 'x<11.25'),
                                                                   right=('x>35', 'y>-11.25', 'y<0'))[task] for p in ('on', 'inside', 'outside')] +
                            ['E|red|%s|l%d' % (p, v) for p in ('on', 'inside', 'outside') for v in (1, 2)] +
                            ['E|dev|%s15|%s' % (s, p) for s in '+-' for p in ('on', 'inside', 'outside')]),
    G=lambda task, counts: ['G|vx%s|%s|%s' % (v, s, p) for v in ('5', '6.3', '0') for s in '+-' for p in ('inside', 'outside')] + ['G|vx0|r1'],
    H=lambda task, counts: ['H|%s' % k for k in ('col+road', 'road+dev', 'dev+stab', 'stab+red', 'red+goal', 'all')],
    I=lambda task, counts: ['I|pair%d|l%gw%g|%s' % (k, np.float32(l), np.float32(w), p) for k in range(4) for l in (4.8, 5.0, 4.2) for w in (2.0, 1.8, 2.2)
                            for p in ('inside', 'outside')])


@pytest.mark.parametrize('name,task,n_veh', FILES, ids=IDS)
def test_every_label_of_families_c_to_i_is_present(name, task, n_veh):
    g = load(name)
    labels = set(str(l) for l in g['label'])
    for fam in ('CD' if n_veh is not None else 'CDEGHI'):
        missing = [l for l in REQUIRED[fam](task, _counts(task, n_veh)) if l not in labels]
        assert not missing, missing
    if n_veh is not None:
        return
    # F: both sides of every wall segment, at the axis headings and at oblique ones
    walls = {}
    for l in labels:
        if l.startswith('F|'):
            _, wall, side, phi = l.split('|')
            walls.setdefault(wall, set()).add((side, float(phi[3:])))
    assert len(walls) == 12 and {w.rstrip('_ab') for w in walls} >= {'lane_lo', 'lane_hi', 'stop_line', 'box_bottom', 'box_top', 'box_left',
                                                                      'box_right', 'exit_lo', 'exit_hi', 'exit_mouth'}, sorted(walls)
    for wall, cases in walls.items():
        phis = {p for _, p in cases}
        assert all(('+d', p) in cases and ('-d', p) in cases for p in phis) and len(phis) >= 3, wall
    all_phis = {p for cases in walls.values() for _, p in cases}
    assert {0.0, 90.0, -90.0, 180.0} <= all_phis and any(p % 90 for p in all_phis)


@pytest.mark.parametrize('task', TASKS)
def test_family_c_inputs_sit_on_the_stop_line_and_on_the_stop_line_car(task):
    g = load('g20_env_edges_%s' % task)
    lit = (g['v_light'] != 0) | (g['virtual'] != 0)
    ey = g['ego'][:, 4]
    for y in (np.float32(-25), EE.up(-25), EE.down(-25)):
        for vl, vf in ((1, 0), (0, 1), (2, 1), (0, 0)):
            if task != 'right':
                assert ((ey == y) & (g['v_light'] == vl) & (g['virtual'] == vf)).any(), (y, vl, vf)
    if task == 'right':
        assert (lit & (ey < -25)).any()
        return
    below = lit & (ey < -25)
    for mode, cx in (('dl', 1.875), ('du', 5.625)):
        mine = g['cand_mode'] == EE.MODES12.index(mode)
        same_y = mine & (g['cand'][:, :, 1] == np.float32(-22.5))
        twin = same_y & (g['cand'][:, :, 0] == np.float32(cx))
        assert (below & (same_y & ~twin).any(1)).any() and (below & twin.any(1)).any(), mode
    # du's own filter against the stop-line car: ego_x + 5 (float32) below, on and one ulp above 5.625
    sums = set((g['ego'][below, 3] + np.float32(5)).tolist())
    assert {5.5, 5.625, float(EE.up(5.625))} <= sums


@pytest.mark.parametrize('task', TASKS)
def test_every_done_code_and_every_adjacent_pair_of_the_chain_occurs(task):
    g = load('g20_env_edges_%s' % task)
    assert set(g['done_code'].tolist()) == set(range(7)) - ({5} if task == 'right' else set())    # E2E:245: a right turn never runs the light
    p = EE.predicates(g, task)
    first = np.where(p.any(1), p.argmax(1) + 1, 0)
    assert np.array_equal(first, g['done_code'])            # the recorded code is the first condition that holds
    for k in range(5):
        if task == 'right' and k in (3, 4):                 # the red-light condition never holds for a right turn
            continue
        both = p[:, k] & p[:, k + 1] & ~p[:, :k].any(1)
        assert both.any(), 'no scene in which conditions %d and %d both hold and none before them' % (k + 1, k + 2)
    assert p.all(1).any() or (task == 'right' and p[:, [0, 1, 2, 3, 5]].all(1).any())
    # E on copied quantities: |delta_y| on 15 and its neighbours, either sign; the ego's y on -25 and its neighbours under a red light
    dy = set(g['done_delta_y'].tolist())
    assert {s * float(v) for s in (1, -1) for v in (np.float32(15), EE.up(15), EE.down(15))} <= dy
    red = g['v_light'] != 0
    assert {float(np.float32(-25)), float(EE.up(-25)), float(EE.down(-25))} <= set(g['ego'][red, 4].tolist())
    # G: |r| at r_bound (1 +- 1e-3), v_x = 0 included
    ratio = np.abs(g['ego'][:, 2].astype(np.float64)) / g['r_bound']
    for vx0 in (True, False):
        rows = (g['ego'][:, 0] == 0) == vx0
        assert (np.abs(ratio[rows] - (1 - 1e-3)) < 1e-4).any() and (np.abs(ratio[rows] - (1 + 1e-3)) < 1e-4).any()


def test_generator_reproduces_a_family_of_the_committed_fixtures():
    from oracle import refload
    if not refload.available():
        pytest.skip('reference tree not present (build container only)')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'oracle', 'gen_golden_env_edges.py'), '--check', 'B'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('reproduced') == 6
