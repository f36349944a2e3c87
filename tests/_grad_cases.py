"""Shared by tests/test_grad_host.py and tests/test_gpu_grad.py: the gradient fixtures (scripts/gen_golden_grad.py) and the
tolerance they carry.

Tolerance (per output column c, over the rows whose flag is set):
    |g - g_float64_ref| <= 4 * E_c + 2**-20 * max_rows |g_float64_ref[:, c]|,   E_c = max_rows |g_float32_ref - g_float64_ref|
The code under test is a second, independent fp32 evaluation of the reference's expressions (its own operation order, its own
sin / cos), so its error is of the size of the reference's own fp32 error; the factor covers a sample maximum over a few hundred
rows; the floor is eight fp32 ulps of the column's magnitude, for columns where the reference's two runs happen to agree.
At most 1 % of a file's rows may carry a cleared flag (a condition on the inputs, not a measurement)."""
import json

import numpy as np

from tests._helpers import golden

TASKS = ('left', 'straight', 'right')
MAX_EXCLUDED = 0.01


class Case(object):
    def __init__(self, z, name, meta):
        self.name, self.meta = name, meta
        self.mode, self.n_veh, self.n_future, self.path_id = meta['mode'], meta['n_veh'], meta['n_future'], meta['path_id']
        self.nd = 9 + 3 * self.n_future
        self._z = z

    def __getitem__(self, k):
        return self._z['%s/%s' % (self.name, k)]

    def ref_idx(self):
        return self['ref_idx'] if self.mode == 'training' else None


def cases(kind, task):
    """kind: 'g15_grad_step' / 'g16_grad_chain' -> list of Case"""
    z = golden('%s_%s' % (kind, task))
    return [Case(z, name, meta) for name, meta in json.loads(str(z['cases'])).items()]


def edge_cases(task):
    """g18_grad_edges_<task>: synthetic edge scenes -> (step cases, laid out as G15's; chain cases, laid out as G16's)"""
    cs = cases('g18_grad_edges', task)
    return [c for c in cs if c.meta['horizon'] is None], [c for c in cs if c.meta['horizon'] is not None]


def step_and_edge_cases(task):
    return cases('g15_grad_step', task) + edge_cases(task)[0]


def chain_and_edge_cases(task):
    return cases('g16_grad_chain', task) + edge_cases(task)[1]


def column_tolerance(E, ref64, ok):
    ref = np.abs(np.asarray(ref64, np.float64).reshape(len(ok), -1, len(E)))[ok]
    return 4.0 * np.asarray(E, np.float64) + 2.0 ** -20 * ref.max((0, 1))


def check_columns(got, ref64, E, ok, what, ratios=None):
    """got / ref64: [B, C] (or [B, H, C]: every step of a row held to column c's bound); -> max |got - ref| / E per column"""
    got = np.asarray(got, np.float64).reshape(len(ok), -1, len(E))[ok]
    ref = np.asarray(ref64, np.float64).reshape(len(ok), -1, len(E))[ok]
    err = np.abs(got - ref).max((0, 1))
    tol = column_tolerance(E, ref64, ok)
    ratio = err / np.maximum(np.asarray(E, np.float64), 1e-300)
    fmt = lambda v: np.array2string(np.asarray(v), precision=2, max_line_width=100000)
    print('%-58s max|g - g64| / E per column: %s   err / tolerance: %s' % (
        what, fmt(np.where(np.asarray(E) > 0, ratio, np.nan)), fmt(err / np.maximum(tol, 1e-300))))
    if ratios is not None:
        ratios[what] = ratio
    assert np.isfinite(got).all(), '%s: non-finite gradient' % what
    assert (err <= tol).all(), '%s: columns %s exceed 4 E + 2^-20 max|g|: err %s, tol %s' % (what, np.nonzero(err > tol)[0], err, tol)


# ---- which branches of rollout_out a G18 step case reaches: recomputed from its stored inputs, float64 NumPy ----
LWS, NEAR_R = 1.4, 6.31      # (L - W) / 2; centres farther apart than 3.5 + 2 LWS have no circle pair below 3.5 m (DAM:228)
# wall name -> (px, py) -> (the circle is in the condition's region, the margin that is compared with 1 m), DAM:233-295 in source
# order.  'x<0,11.25-y<1' is the band -25 <= x < 0, where veh2road4training has the term and veh2road4real has none (DAM:239 / 248).
WALLS = {
    'left': [('y<-25,x<1', lambda x, y: (y < -25.0, x)), ('y<-25,3.75-x<1', lambda x, y: (y < -25.0, 3.75 - x)),
             ('x<0,11.25-y<1', lambda x, y: ((x < 0.0) & ~(x < -25.0), 11.25 - y)),
             ('x<-25,11.25-y<1', lambda x, y: (x < -25.0, 11.25 - y)), ('x<-25,y<1', lambda x, y: (x < -25.0, y))],
    'straight': [('y<-25,x-3.75<1', lambda x, y: (y < -25.0, x - 3.75)), ('y<-25,7.5-x<1', lambda x, y: (y < -25.0, 7.5 - x)),
                 ('y>25,11.25-x<1', lambda x, y: (y > 25.0, 11.25 - x)), ('y>25,x<1', lambda x, y: (y > 25.0, x))],
    'right': [('y<-25,x-7.5<1', lambda x, y: (y < -25.0, x - 7.5)), ('y<-25,11.25-x<1', lambda x, y: (y < -25.0, 11.25 - x)),
              ('x>25,-y<1', lambda x, y: (x > 25.0, -y)), ('x>25,y+11.25<1', lambda x, y: (x > 25.0, y + 11.25))],
}


def grid_box(task):
    """the closest-point cell grid of the forward: the paths' bounding box and 20 m (csrc/eb_capi.hip: build_cell_grid)"""
    from env_build_amd.ref_path_tables import build_ref_paths
    pts = np.concatenate([np.stack([np.asarray(p[0], np.float64), np.asarray(p[1], np.float64)], 1) for p in build_ref_paths(task)[0]])
    return np.floor(pts.min(0) - 20.0), pts.max(0) + 20.0


def edge_census(task, c):
    """branch name -> bool [B]: the rows of step case c that take it"""
    o, a = c['obs'].astype(np.float64), np.clip(c['actions'].astype(np.float64), -1.05, 1.05)
    B, took = len(o), {}
    v_x, v_y, r, x, y, phi = o[:, 0], o[:, 1], o[:, 2], o[:, 3], o[:, 4], o[:, 5] * np.pi / 180.0
    front, rear = (x + LWS * np.cos(phi), y + LWS * np.sin(phi)), (x - LWS * np.cos(phi), y - LWS * np.sin(phi))
    for name, f in WALLS[task]:
        (rf, mf), (rr, mr) = f(*front), f(*rear)
        on_f, on_r = rf & (mf < 1.0), rr & (mr < 1.0)
        took['wall %s: front' % name], took['wall %s: rear' % name] = on_f & ~on_r, on_r & ~on_f
        took['wall %s: both' % name] = on_f & on_r
        took['wall %s: far side' % name] = rf & (mf >= 1.0) & (mf < 1.3) & ~on_r            # in the region, margin just >= 1 m
        took['wall %s: out of the region' % name] = ~rf & ~rr & (mf < 1.0) & (mr < 1.0)     # margins < 1 m, region not entered
    a_x = 2.25 * a[:, 1] - 0.75                                                            # DAM:131
    nx0 = v_x + 0.1 * (a_x + v_y * r)                                                      # DAM:73, before the clip of DAM:390
    took.update({'v_x below 0': nx0 < 0.0, 'v_x above 35': nx0 > 35.0, 'v_x just inside 0': (nx0 >= 0.0) & (nx0 < 0.3),
                 'v_x just inside 35': (nx0 <= 35.0) & (nx0 > 34.7), 'action clipped': (np.abs(c['actions']) > 1.05).any(1)})
    if task != 'straight':                                                                 # two2one of the NEXT pose, DAM:740-741 / 750-751
        nx, ny = x + 0.1 * (v_x * np.cos(phi) - v_y * np.sin(phi)), y + 0.1 * (v_x * np.sin(phi) + v_y * np.cos(phi))
        after = nx < -25.0 if task == 'left' else nx > 25.0
        took.update({'two2one before': (ny < -25.0) & ~after, 'two2one arc': ~(ny < -25.0) & ~after, 'two2one after': after})
    veh = o[:, c.nd:].reshape(B, c.n_veh, 4)
    near = np.sqrt((x[:, None] - veh[:, :, 0]) ** 2 + (y[:, None] - veh[:, :, 1]) ** 2) < NEAR_R
    vphi = veh[:, :, 3] * np.pi / 180.0
    below35 = below25 = 0
    for px, py in (front, rear):
        for sgn in (1.0, -1.0):
            d = np.sqrt((px[:, None] - (veh[:, :, 0] + sgn * LWS * np.cos(vphi))) ** 2 + (py[:, None] - (veh[:, :, 1] + sgn * LWS * np.sin(vphi))) ** 2)
            below35, below25 = below35 + (d < 3.5).sum(1), below25 + (d < 2.5).sum(1)
    crowded = near.all(1) & (below35 >= c.n_veh) & (below25 >= c.n_veh // 4)
    took.update({'crowded, 32 slots': crowded & (c.n_veh == 32), 'crowded, 64 slots': crowded & (c.n_veh == 64),
                 'no vehicle near, 32 or 64 slots': ~near.any(1) & (c.n_veh >= 32)})
    lo, hi = grid_box(task)
    p = np.stack([x, y], 1)
    outside = ((p < lo) | (p > hi)).any(1)
    edge = np.minimum(np.abs(p - lo), np.abs(p - hi))                                        # distance to the box's four lines
    on_border = (((edge[:, 0] < 1.0) & (p[:, 1] >= lo[1] - 1.0) & (p[:, 1] <= hi[1] + 1.0))
                 | ((edge[:, 1] < 1.0) & (p[:, 0] >= lo[0] - 1.0) & (p[:, 0] <= hi[0] + 1.0)))
    took.update({'ego off the cell grid': outside & ~on_border, 'ego beyond 200 m': np.abs(p).max(1) > 200.0,
                 'ego on the grid border': on_border})
    if c.mode == 'training':
        took['ref_idx out of range'] = (c['ref_idx'] < 0) | (c['ref_idx'] > 2)
    took['near records'] = near.sum(1)
    return took


# ---- the one documented divergence: a circle distance of exactly zero (sqrt'(0): NaN in the reference, 0 here) ----
def zero_distance_case(task):
    """The G18 rows with no vehicle near and an ego heading of exactly 90 degrees, slot 0's vehicle moved onto the ego with the ego's
    heading: circle pairs (front, front) and (rear, rear) at distance exactly 0, the cross pairs at 2 LWS = 2.8 m.
    -> case, row indices, obs with the vehicle moved, expected d L / d obs [rows, nd] in float64.

    Expected: the fixture's g_obs64 of the row (the moved vehicle was beyond every threshold, the vehicle columns carry no cotangent)
    plus the two cross pairs' part, DAM:218-229 differentiated by hand.  With u = (cos phi, sin phi), ego points F = P + LWS u and
    R = P - LWS u and the vehicle's F' = F, R' = R: d(F, R') = d(R, F') = 2 LWS < 3.5, >= 2.5, so only veh2veh4training
    (cotangent w = g_out5[1]) has the term (d - 3.5)^2 per pair; its gradient with respect to the ego point is
    2 w (d - 3.5) (point - other) / d = k u at F and -k u at R, k = 2 w (2 LWS - 3.5).  x and y get their sum; the heading (radians) gets
    LWS ((gF - gR) . (-sin phi, cos phi)); obs column 5 is in degrees."""
    c = [c for c in edge_cases(task)[0] if c.name.startswith('crowded') and c.n_veh == 32][0]
    took = edge_census(task, c)
    rows = np.nonzero(took['no vehicle near, 32 or 64 slots'] & (c['obs'][:, 5] == 90.0) & c['ok'])[0]
    assert len(rows) >= 8
    obs = c['obs'].copy()
    obs[rows, c.nd + 0], obs[rows, c.nd + 1], obs[rows, c.nd + 3] = obs[rows, 3], obs[rows, 4], obs[rows, 5]
    # the distances in the forward's working precision: the vehicle's circle centres are the ego's, float for float
    f = np.float32
    phi = (obs[rows, 5] * f(np.pi) / f(180.0)).astype(f)
    cs, sn = np.cos(phi).astype(f), np.sin(phi).astype(f)
    for sgn in (f(1.0), f(-1.0)):
        ex, ey = obs[rows, 3] + sgn * f(LWS) * cs, obs[rows, 4] + sgn * f(LWS) * sn
        vx, vy = obs[rows, c.nd] + sgn * f(LWS) * cs, obs[rows, c.nd + 1] + sgn * f(LWS) * sn
        assert (np.sqrt((ex - vx) ** 2 + (ey - vy) ** 2) == 0.0).all()
    phi64 = obs[rows, 5].astype(np.float64) * np.pi / 180.0
    u = np.stack([np.cos(phi64), np.sin(phi64)], 1)
    d = 2.0 * LWS
    k = 2.0 * c['g_out5'][1, rows].astype(np.float64) * (d - 3.5)
    gF, gR = k[:, None] * (2.0 * LWS * u) / d, k[:, None] * (-2.0 * LWS * u) / d
    want = c['g_obs64'][rows].copy()
    want[:, 3:5] += gF + gR
    normal = np.stack([-u[:, 1], u[:, 0]], 1)
    want[:, 5] += LWS * ((gF - gR) * normal).sum(1) * np.pi / 180.0
    return c, rows, obs, want


def check_zero_distance(c, rows, go, ga, want, what):
    """finite everywhere; the moved rows within the case's own column tolerance of the closed form, every other row as the fixture"""
    assert np.isfinite(go).all() and np.isfinite(ga).all(), what
    ref = c['g_obs64'].copy()
    ref[rows] = want
    check_columns(go, ref, c['E_obs'], c['ok'], what + ' obs')
    check_columns(ga, c['g_act64'], c['E_act'], c['ok'], what + ' act')
    tol = column_tolerance(c['E_obs'], c['g_obs64'], c['ok'])
    assert (np.abs(np.asarray(go, np.float64)[rows] - want) <= tol).all(), what
