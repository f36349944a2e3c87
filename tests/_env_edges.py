"""The env-side rules of fixture G20 (tests/golden/g20_env_edges_<task>.npz, g20w_env_edges_<task>_N16.npz) restated as tables in
NumPy — used by the generator (oracle/gen_golden_env_edges.py) to PLACE vehicles and egos, and by the census test
(tests/test_env_edges_census.py) to prove from the fixture's inputs alone that every case it is meant to hold is still there.
Nothing here is used as an expectation of a replay: the expectations are the reference's recorded outputs."""
import numpy as np

MODES12 = ('dl', 'du', 'dr', 'rd', 'rl', 'ru', 'ur', 'ud', 'ul', 'lu', 'lr', 'ld')      # = _capi.VMODE_ID's order
VACANT = 255
MODE_COUNTS = dict(left=dict(dl=2, du=2, ud=2, ul=2), straight=dict(dl=1, du=2, ud=2, ru=2, ur=2), right=dict(dr=1, ur=2, lr=2))   # UTL:21-23
DONE_NAMES = ('not_done_yet', 'collision', 'break_road_constrain', 'deviate_too_much', 'break_stability', 'break_red_light', 'good_done')
FAMILIES = 'ABCDEFGHI'
F32 = np.float32


def f32(v):
    return np.float32(v)


def up(v):
    return np.nextafter(F32(v), F32(np.inf))


def down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def tiled_counts(task, n_veh):
    """slot list of the project for n_veh slots (the native list tiled) -> (slot modes, count per mode in the native order)"""
    base = [m for m, k in MODE_COUNTS[task].items() for _ in range(k)]
    slots = [base[i % len(base)] for i in range(n_veh)]
    return slots, {m: slots.count(m) for m in MODE_COUNTS[task]}


def filter_bounds(task, mode, ex, ey):
    """E2E:393-411 as data: [(name, axis 0 = x / 1 = y, side, value)], side '>' = the coordinate must be strictly greater.  Ego-relative
    values are float32 operations on the float32 ego, as the reference's are (ego_dynamics holds numpy.float32 scalars)."""
    ex, ey = F32(ex), F32(ey)
    t = dict(dl=[('x>-35', 0, '>', F32(-35)), ('y>ey-2', 1, '>', ey - F32(2))],
             du=[('y>ey-2', 1, '>', ey - F32(2)), ('y<35', 1, '<', F32(35)), ('x<ex+5', 0, '<', ex + F32(5))],
             dr=[('x<35', 0, '<', F32(35)), ('y>ey', 1, '>', ey)],
             ru=[('x<35', 0, '<', F32(35)), ('y<35', 1, '<', F32(35))],
             ud=[('y>max(ey-2,-25)', 1, '>', max(ey - F32(2), F32(-25))), ('y<25', 1, '<', F32(25)), ('x<ex', 0, '<', ex)],
             ul=[('x>-35', 0, '>', F32(-35)), ('x<ex', 0, '<', ex), ('y<25', 1, '<', F32(25))],
             lr=[('x>-35', 0, '>', F32(-35)), ('x<35', 0, '<', F32(35))])
    if mode == 'ur':
        return {'straight': [('x<ex+7', 0, '<', ex + F32(7)), ('y>ey', 1, '>', ey), ('y<35', 1, '<', F32(35))],
                'right': [('x<35', 0, '<', F32(35)), ('y<25', 1, '<', F32(25))]}.get(task, [])
    return t.get(mode, [])


def in_range(task, mode, ex, ey, x, y, skip=None):
    ok = True
    for name, axis, side, val in filter_bounds(task, mode, ex, ey):
        if name == skip:
            continue
        c = F32((x, y)[axis])
        ok = ok and bool(c > val if side == '>' else c < val)
    return ok


# E2E:414-428 as data: [(axis, +1 ascending / -1 descending)]; equal keys keep their insertion order (sorted() is stable, with
# reverse=True too)
def sort_keys(task, mode):
    if mode == 'ur':
        return {'straight': [(1, 1)], 'right': [(1, 1), (0, -1)]}.get(task, [])
    return dict(dl=[(1, 1), (0, -1)], du=[(1, 1)], dr=[(1, 1), (0, 1)], ru=[(0, 1), (1, -1)], ud=[(1, 1)], ul=[(1, 1), (0, 1)],
                lr=[(0, -1)]).get(mode, [])


def stop_line_car(task, mode, ey, lit):
    """E2E:386-390 -> (x, y) of the appended car or None"""
    if task == 'right' or not lit or not F32(ey) < F32(-25) or mode not in ('dl', 'du'):
        return None
    return (1.875, -22.5) if mode == 'dl' else (5.625, -22.5)


def ranked(task, mode, ex, ey, lit, cand, cmode):
    """the in-range members of one mode in the reference's order -> [(candidate index or len(cand) for the stop-line car, x, y)]"""
    rows = [(c, float(cand[c, 0]), float(cand[c, 1])) for c in range(len(cand)) if cmode[c] == MODES12.index(mode)]
    car = stop_line_car(task, mode, ey, lit)
    if car is not None:
        rows.append((len(cand), car[0], car[1]))
    rows = [r for r in rows if in_range(task, mode, ex, ey, r[1], r[2])]
    keys = sort_keys(task, mode)
    return sorted(rows, key=lambda r: tuple(s * (r[1], r[2])[a] for a, s in keys))     # stable: ties stay in insertion order


def feasible(x, y, task):
    from env_build_amd.endtoend_env_utils import judge_feasible
    return judge_feasible(float(x), float(y), task)


def predicates(g, task):
    """the six conditions of _judge_done (E2E:208-256) per scene, in priority order, from the fixture's inputs (the collision flag,
    the corner points and r_bound are the recorded quantities the reference itself decides on) -> bool [n, 6]"""
    ego, n = g['ego'], len(g['ego'])
    road = np.array([not all(feasible(cx, cy, task) for cx, cy in g['corners'][i]) for i in range(n)])
    dev = np.abs(g['done_delta_y'].astype(np.float32)) > 15
    rb = g['r_bound'].astype(np.float32)
    stab = ~((-rb < ego[:, 2]) & (ego[:, 2] < rb))
    red = (g['v_light'] != 0) & (ego[:, 4] > -25) & (task != 'right')
    x, y = ego[:, 3], ego[:, 4]
    goal = {'left': (x < -35) & (0 < y) & (y < 11.25), 'right': (x > 35) & (-11.25 < y) & (y < 0),
            'straight': (y > 35) & (0 < x) & (x < 11.25)}[task]
    return np.stack([g['collision'] != 0, road, dev, stab, red, goal], 1)


def regroup(block, task, n_veh):
    """the reference's vehicle block (modes in dict order, counts of tiled_counts) -> the project's slot order: rank r of mode m goes
    to the r-th slot of mode m"""
    slots, counts = tiled_counts(task, n_veh)
    rows = np.asarray(block).reshape(len(block), n_veh, 4)
    start, at = {}, 0
    for m, k in counts.items():
        start[m] = at
        at += k
    seen, out = {m: 0 for m in counts}, np.empty_like(rows)
    for s, m in enumerate(slots):
        out[:, s] = rows[:, start[m] + seen[m]]
        seen[m] += 1
    return out.reshape(len(block), 4 * n_veh)
