"""The penalty sums' two summation orders, stated a second time, and the scenes that tell them apart (not collected).

resum() re-associates the fp32 terms the oracle exports (HostModel.penalty_terms) in NumPy float32, one addition at a time:
  'reference'  one running sum over slots and, inside a slot, over ff, fr, rf, rr — DAM:218-229;
  'record'     per slot ((ff + fr) + rf) + rr, the partials joined in slot order — every HIP kernel.
Both end with `+ road` (DAM:299-300).  The oracle's switch is held to THIS text (tests/test_penalty_order_host.py), the kernels
to the oracle (tests/test_gpu_penalty_order.py).

scenes() builds observation rows (n_future = 0) whose penalty sums are made of known numbers of terms: see its docstring.
"""
import numpy as np

F = np.float32
LWS = F((4.8 - 2.0) / 2.)           # circle offset along the axis of a vehicle (DAM:210)
PAIRS = ('ff', 'fr', 'rf', 'rr')    # ego circle, vehicle circle: the order of the four terms of a record
MAX_ROWS = 1024


def resum(t35, t25, road, order):
    """terms [n, n_veh, 4] x 2, road [n, 2] -> (v2v_train, v2v_real, punish_train, punish_real), float32 [n] each"""
    assert order in ('reference', 'record')
    t35, t25, road = np.asarray(t35), np.asarray(t25), np.asarray(road)
    assert t35.dtype == F and t25.dtype == F and road.dtype == F and t35.shape == t25.shape and t35.shape[2] == 4
    out = []
    with np.errstate(all='ignore'):
        for t in (t35, t25):
            acc = np.zeros(t.shape[0], F)
            for j in range(t.shape[1]):
                if order == 'record':
                    part = t[:, j, 0] + t[:, j, 1]
                    part = part + t[:, j, 2]
                    part = part + t[:, j, 3]
                    acc = acc + part
                else:
                    for k in range(4):
                        acc = acc + t[:, j, k]
            assert acc.dtype == F
            out.append(acc)
        return out[0], out[1], out[0] + road[:, 0], out[1] + road[:, 1]


def expected_out5_rows(t35, t25, road, order):
    """-> rows 1..4 of out5 ([4, n]) and rows 12..15 of the reward dictionary ([4, n]) from the terms"""
    vt, vr, pt, pr = resum(t35, t25, road, order)
    return np.stack([pt, pr, vr, road[:, 1]]), np.stack([vt, road[:, 0], vr, road[:, 1]])


# the walls of each task as (x, y, heading in degrees) of an ego whose two circle centres both collect that wall's term
# (DAM:233-295); the fifth pose of 'left' collects the training-only wall (px < 0 where the real sum asks px < -25)
WALL_POSES = {
    'left': [(0.5, -30.0, 90.0), (3.2, -30.0, 90.0), (-30.0, 10.8, 180.0), (-30.0, 0.4, 180.0), (-10.0, 10.8, 180.0)],
    'straight': [(4.2, -30.0, 90.0), (7.0, -30.0, 90.0), (10.8, 30.0, 90.0), (0.4, 30.0, 90.0)],
    'right': [(8.0, -30.0, 90.0), (10.8, -30.0, 90.0), (30.0, -0.5, 0.0), (30.0, -10.8, 0.0)],
}


def _unit(deg):
    r = np.deg2rad(deg)
    return np.array([np.cos(r), np.sin(r)])


def _f32_neighbours(x, k=3):
    """the float32 nearest x with its k predecessors and k successors"""
    c = F(x)
    lo, hi, out = c, c, [c]
    for _ in range(k):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return sorted(float(v) for v in out)


class _Rows(object):
    def __init__(self, n_veh, rng):
        self.n_veh, self.rng = n_veh, rng
        self.ego, self.veh, self.block, self.meta = [], [], [], []

    def far(self, ego_xy):
        """every slot 30 .. 60 m from the ego: no term, and none after a few steps of any rollout either"""
        r, a = self.rng.uniform(30, 60, self.n_veh), self.rng.uniform(-np.pi, np.pi, self.n_veh)
        v = np.zeros((self.n_veh, 4))
        v[:, 0], v[:, 1] = ego_xy[0] + r * np.cos(a), ego_xy[1] + r * np.sin(a)
        v[:, 2], v[:, 3] = self.rng.uniform(0, 8, self.n_veh), -self.rng.uniform(-180, 180, self.n_veh)
        return v

    def add(self, block, ego_xy, ego_phi, placed, meta=None, ego_v=None):
        """placed: {slot: (x, y, v, phi)}; the other slots far away"""
        veh = self.far(ego_xy)
        for j, rec in placed.items():
            veh[j] = rec
        v_x = self.rng.uniform(0, 8) if ego_v is None else ego_v
        self.ego.append([v_x, 0.0, 0.0, ego_xy[0], ego_xy[1], ego_phi])
        self.veh.append(veh)
        self.block.append(block)
        self.meta.append(meta)


def _lone_record(rng, ego_xy, ego_phi, pair, d):
    """a record whose circle pair `pair` is d apart and whose other three pairs are more than 3.5 m apart: the vehicle circle
    lies beyond the ego circle, within 30 degrees of the ego's axis, and the vehicle's other circle beyond that, within 30
    degrees of the same line (so every other distance is at least |2.8 n0 + d n| > 3.5 for d > 1)"""
    out = 0.0 if pair[0] == 'f' else 180.0                    # outward direction of the ego circle along the ego's axis
    p = np.asarray(ego_xy) + float(LWS) * _unit(ego_phi + out)
    n_deg = ego_phi + out + rng.uniform(-30, 30)
    q = p + d * _unit(n_deg)
    m_deg = n_deg + rng.uniform(-30, 30)                      # from the near vehicle circle to the vehicle's other circle
    v_phi = m_deg + 180.0 if pair[1] == 'f' else m_deg
    c = q + float(LWS) * _unit(m_deg)
    v_phi = (v_phi + 180.0) % 360.0 - 180.0
    return (c[0], c[1], rng.uniform(0, 8), v_phi)


def _mid_ego(rng):
    """an ego in the middle of the junction: no wall of any task is within reach of its circles"""
    return (rng.uniform(0.5, 3.5), rng.uniform(-4, 4)), rng.uniform(-180, 180)


def scenes(task, n_veh, seed):
    """-> dict(obs [n, 9 + 4 n_veh] float32, ref_idx [n] int32, actions [8, n, 2], block [n] of str, rows = {block: indices},
               centre_distance [n] (NaN outside the boundary block), meta [n]: what a row was built for — (pair, slot) of a lone
               pair, the vehicle count of a dense row, the wall of a wall row), n <= 1024.

    Blocks (every block but 'walls' keeps the ego in the middle of the junction, where the road sums are exactly 0):
      lone35 / lone25   one vehicle, exactly one circle pair under 3.5 m (under 2.5 m), for each of ff / fr / rf / rr, the
                        vehicle's slot cycling through 0 .. n_veh - 1 (bit 63 of the fused kernel's slot mask at n_veh = 64)
      boundary          both headings along the line of centres (only ego-front / vehicle-rear can be close), the centre distance
                        on 6.25 .. 6.40 m by 2.5 mm plus the float32 neighbours of 6.3 (3.5 + 2.8) and of sqrt(40.5), the near
                        filter's radius; the same around 5.3 m (2.5 + 2.8)
      two_in_record     two terms in one record;  two_records: one term each in slots 0 and n_veh - 1
      dense             4, 8, ... , all n_veh vehicles within 3 m of the ego: the rows on which the two orders differ
      walls             the ego's circles collect the road terms of each wall of the task, some vehicles near as well
      nonfinite         inf / NaN / 2e38 in record fields of a dense row
    """
    rng = np.random.default_rng([seed, n_veh, ('left', 'straight', 'right').index(task)])
    R = _Rows(n_veh, rng)
    # ---- lone pair ----
    reps = max(1, min(n_veh, 64))
    k = 0
    for block, lo, hi in (('lone35', 2.6, 3.45), ('lone25', 1.1, 2.45)):
        for pair in PAIRS:
            for _ in range(reps):
                xy, phi = _mid_ego(rng)
                slot = k % n_veh
                k += 1
                R.add(block, xy, phi, {slot: _lone_record(rng, xy, phi, pair, rng.uniform(lo, hi))}, meta=(pair, slot))
    # ---- boundary: ego at the origin heading along +x (cos = 1, sin = 0 exactly), the vehicle on the x axis heading +x, so that
    #      its x IS the centre distance in float32 ----
    cds = []
    for c0 in (6.3, 5.3):
        cds += [c0 - 0.05 + 0.0025 * i for i in range(41)] + [c0 + 0.05 + 0.0025 * i for i in range(1, 21)]
        cds += _f32_neighbours(c0)
    cds += _f32_neighbours(np.sqrt(40.5))
    cds += [6.3 + 1e-3, float(np.nextafter(F(6.3 + 1e-3), F(0)))]
    for i, cd in enumerate(cds):
        cd = float(F(cd))
        R.add('boundary', (0.0, 0.0), 0.0, {i % n_veh: (cd, 0.0, rng.uniform(0, 8), 0.0)}, meta=cd)
    # ---- two terms ----
    for i in range(32):
        xy, phi = _mid_ego(rng)
        h = rng.uniform(1.0, 1.5) if i % 4 == 3 else rng.uniform(2.5, 2.9)
        side = 1.0 if i % 2 else -1.0                                       # the vehicle stands beside the ego, its axis across
        q = np.asarray(xy) + rng.uniform(-0.5, 0.5) * _unit(phi) + side * h * _unit(phi + 90.0)
        front_near = (i // 2) % 2 == 0                                      # which of the vehicle's circles is the near one
        away = phi + side * 90.0
        c = q + float(LWS) * _unit(away)
        v_phi = away + 180.0 if front_near else away
        R.add('two_in_record', xy, phi, {i % n_veh: (c[0], c[1], rng.uniform(0, 8), (v_phi + 180.0) % 360.0 - 180.0)})
    if n_veh >= 2:
        for i in range(32):
            xy, phi = _mid_ego(rng)
            pa, pb = ('ff', 'rr') if i % 2 else ('fr', 'rf')
            lo, hi = (1.1, 2.45) if i % 4 == 3 else (2.6, 3.45)
            R.add('two_records', xy, phi, {0: _lone_record(rng, xy, phi, pa, rng.uniform(lo, hi)),
                                           n_veh - 1: _lone_record(rng, xy, phi, pb, rng.uniform(lo, hi))})

    def crowd(xy, count):
        slots = rng.choice(n_veh, size=count, replace=False)
        r, a = 3.0 * np.sqrt(rng.random(count)), rng.uniform(-np.pi, np.pi, count)
        return {int(j): (xy[0] + r[i] * np.cos(a[i]), xy[1] + r[i] * np.sin(a[i]), rng.uniform(0, 2.0), -rng.uniform(-180, 180))
                for i, j in enumerate(slots)}
    # ---- dense ----
    counts = sorted(set(list(range(4, n_veh + 1, 4)) + [n_veh]))
    per = max(2, min(8, 96 // len(counts)))
    for count in counts:
        for _ in range(per):
            xy, phi = _mid_ego(rng)
            R.add('dense', xy, phi, crowd(xy, count), meta=count)
    # ---- walls ----
    for w, (x, y, phi) in enumerate(WALL_POSES[task]):
        for i in range(8):
            xy = (x + rng.uniform(-0.3, 0.3), y + rng.uniform(-0.3, 0.3))
            R.add('walls', xy, phi + rng.uniform(-10, 10), crowd(xy, min(n_veh, (0, 1, 3, n_veh)[i % 4])), meta=w, ego_v=rng.uniform(0, 3))
    # ---- non-finite record fields, as tests/test_gpu_parity.py::test_tape_kernel_crowded_remote_and_special_values plants them ----
    for i, (col, val) in enumerate([(2, np.inf), (3, -np.inf), (3, 2e38), (3, np.nan), (2, np.inf), (3, np.inf)]):
        xy, phi = _mid_ego(rng)
        placed = crowd(xy, min(n_veh, 4))
        slots = sorted(placed)
        for j in (slots[:1] if i < 4 else slots):
            rec = list(placed[j])
            rec[col] = val
            placed[j] = tuple(rec)
        R.add('nonfinite', xy, phi, placed)

    n = len(R.ego)
    assert n <= MAX_ROWS, n
    with np.errstate(over='ignore'):
        ego, veh = np.asarray(R.ego, F), np.asarray(R.veh, np.float64).astype(F)
    trk = rng.uniform(-1, 1, (n, 3)).astype(F)            # (the tracking columns feed the reward, not the penalty sums)
    obs = np.ascontiguousarray(np.concatenate([ego, trk, veh.reshape(n, 4 * n_veh)], axis=1), F)
    block = np.asarray(R.block)
    rows = {b: np.flatnonzero(block == b) for b in dict.fromkeys(R.block)}
    cd = np.full(n, np.nan)
    cd[rows['boundary']] = [R.meta[i] for i in rows['boundary']]
    return dict(obs=obs, ref_idx=rng.integers(0, 3, n).astype(np.int32), block=block, rows=rows, centre_distance=cd,
                meta=R.meta, actions=rng.uniform(-1, 1, (8, n, 2)).astype(F))


ORDER_FREE = ('lone35', 'lone25', 'two_in_record', 'two_records')     # at most two non-zero terms per sum: any order, same bits
