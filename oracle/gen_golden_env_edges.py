#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — fixture G20: the env-side logic (which vehicles an ego sees, in which order, why its episode ends) on
hand-made edge scenes, from the reference's own Python through the seam G6 uses (oracle/gen_golden.py: g6_env_logic):
E2E.CrossroadEnd2end(task, 0, multi_display=True) with all_vehicles / ego_dynamics / v_light / virtual_red_light_vehicle injected,
_get_obs() and _judge_done() called, TRF.Traffic.collision_check called unbound.

  tests/golden/g20_env_edges_<task>.npz        families A-I at the native slot list, 24 candidates per scene
  tests/golden/g20w_env_edges_<task>_N16.npz   families A-D with UTL.VEHICLE_MODE_DICT[task]'s counts widened in place to what
                                               n_veh = 16 gives the project; the vehicle block regrouped into the project's slot
                                               order (rank r of mode m -> the r-th slot of mode m), the slot list stored

Families (the scene's case is in `label`, 'family|...'):
  A filter bounds (on / one ulp inside / one ulp outside; float32 ego arithmetic, exact and inexact)   B sort ties and the slice
  C the stop-line car   D counts and vacant rows   E done rules on copied quantities   F walls, by margin   G stability, by margin
  H the priority chain   I collision circles, by margin
The arrays are G6's plus `label` and `done_delta_y` (the obs[6] _judge_done saw: the generator sets it itself in E and H; elsewhere
it is obs[:, 6]).  Where vehicles and egos are placed is decided with the tables of tests/_env_edges.py; every expectation is the
reference's recorded output.

Regenerate:  python oracle/gen_golden_env_edges.py        (needs the reference tree; deterministic: every family draws from its
own seeded stream, two runs give identical arrays — tests/test_env_edges_census.py regenerates one family and compares)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import gen_golden as GG  # noqa: E402  (loads the reference through oracle/refload.py)
from tests import _env_edges as EE  # noqa: E402

DAM, UTL, E2E, TRF = GG.DAM, GG.UTL, GG.E2E, GG.TRF
TASKS = GG.TASKS
M = 24
D_MARGIN = 1e-3                      # F, I: 50x the 2e-5 m the corner-point checks allow between float64 and fp32 corners
R_MARGIN = 1e-3                      # G: 100x the relative 1e-5 the r_bound check allows
F32 = np.float32
LANE_X = dict(left=1.875, straight=5.625, right=9.375)
LW_SET = [(l, w) for l in (4.8, 5.0, 4.2) for w in (2.0, 1.8, 2.2)]          # the (l, w) values G6 draws from
HEADINGS = (0.0, 90.0, -90.0, 180.0, 33.7, -127.3, 80.4, -99.1, 170.2, 8.6)
GOAL = dict(left=([('x<-35', 0, '<', -35.0), ('y>0', 1, '>', 0.0), ('y<11.25', 1, '<', 11.25)], (-40.0, 5.625, 180.0)),
            straight=([('y>35', 1, '>', 35.0), ('x>0', 0, '>', 0.0), ('x<11.25', 0, '<', 11.25)], (5.625, 40.0, 90.0)),
            right=([('x>35', 0, '>', 35.0), ('y>-11.25', 1, '>', -11.25), ('y<0', 1, '<', 0.0)], (40.0, -5.625, 0.0)))
# judge_feasible's wall segments (UTL:73-104): (name, axis of the wall's normal, its coordinate, the range along it, the side a corner
# is feasible on: +1 / -1, or 0 where both sides are (the stop line: y <= -25 is the lane's, -25 < y the box's; the exit leg's mouth))
WALLS = dict(
    left=[('lane_lo', 0, 0.0, (-45, -27), 1), ('lane_hi', 0, 3.75, (-45, -27), -1), ('stop_line', 1, -25.0, (0.3, 3.45), 0),
          ('box_bottom_a', 1, -25.0, (-24, -1), 1), ('box_bottom_b', 1, -25.0, (4.75, 24), 1), ('box_right', 0, 25.0, (-24, 24), -1),
          ('box_top', 1, 25.0, (-24, 24), -1), ('box_left_a', 0, -25.0, (-24, -1), 1), ('box_left_b', 0, -25.0, (12.25, 24), 1),
          ('exit_lo', 1, 0.0, (-45, -27), 1), ('exit_hi', 1, 11.25, (-45, -27), -1), ('exit_mouth', 0, -25.0, (0.3, 10.95), 0)],
    straight=[('lane_lo', 0, 3.75, (-45, -27), 1), ('lane_hi', 0, 7.5, (-45, -27), -1), ('stop_line', 1, -25.0, (4.05, 7.2), 0),
              ('box_bottom_a', 1, -25.0, (-24, 2.75), 1), ('box_bottom_b', 1, -25.0, (8.5, 24), 1), ('box_right', 0, 25.0, (-24, 24), -1),
              ('box_left', 0, -25.0, (-24, 24), 1), ('box_top_a', 1, 25.0, (-24, -1), -1), ('box_top_b', 1, 25.0, (12.25, 24), -1),
              ('exit_lo', 0, 0.0, (27, 45), 1), ('exit_hi', 0, 11.25, (27, 45), -1), ('exit_mouth', 1, 25.0, (0.3, 10.95), 0)],
    right=[('lane_lo', 0, 7.5, (-45, -27), 1), ('lane_hi', 0, 11.25, (-45, -27), -1), ('stop_line', 1, -25.0, (7.8, 10.95), 0),
           ('box_bottom_a', 1, -25.0, (-24, 6.5), 1), ('box_bottom_b', 1, -25.0, (12.25, 24), 1), ('box_left', 0, -25.0, (-24, 24), 1),
           ('box_top', 1, 25.0, (-24, 24), -1), ('box_right_a', 0, 25.0, (-24, -12.25), -1), ('box_right_b', 0, 25.0, (1, 24), -1),
           ('exit_lo', 1, -11.25, (27, 45), 1), ('exit_hi', 1, 0.0, (27, 45), -1), ('exit_mouth', 0, 25.0, (-10.95, -0.3), 0)])


class widened(object):
    """UTL.VEHICLE_MODE_DICT[task]'s counts -> those of the project's n_veh-slot list, in place (the reference's slice_or_fill reads
    them, E2E:450-451) — as gen_golden.tiled_modes does for VEHICLE_MODE_LIST."""

    def __init__(self, task, n_veh):
        self.task, self.n_veh = task, n_veh

    def __enter__(self):
        d = UTL.VEHICLE_MODE_DICT[self.task]
        assert E2E.VEHICLE_MODE_DICT[self.task] is d
        self.saved = list(d.items())
        if self.n_veh is not None:
            for m, k in EE.tiled_counts(self.task, self.n_veh)[1].items():
                d[m] = k
        return dict(d)

    def __exit__(self, *a):
        for m, k in self.saved:
            UTL.VEHICLE_MODE_DICT[self.task][m] = k


def wrap180(d):
    while d > 180:
        d -= 360
    while d <= -180:
        d += 360
    return d


class Builder(object):
    def __init__(self, task, counts, seed):
        self.task, self.counts, self.seed = task, counts, seed
        self.env = E2E.CrossroadEnd2end(task, 0, multi_display=True)
        self.env.traffic = SimpleNamespace(collision_flag=False)
        self.paths = [DAM.ReferencePath(task, k) for k in range(3)]
        self.n_slots = sum(counts.values())
        self.rec = dict(ego=[], params=[], cand=[], cand_mode=[], cand_lw=[], v_light=[], virtual=[], ref_index=[], obs=[], r_bound=[],
                        corners=[], done_code=[], collision=[], done_delta_y=[], label=[])
        self.k = 0

    # ---- vehicles -----------------------------------------------------------------------------------------------------------
    def veh(self, mode, x, y, lw=(4.8, 2.0)):
        """a candidate with a (v, phi) pair no other of its scene has: the order is visible in the output"""
        k = self.k
        self.k += 1
        return dict(mode=mode, x=float(F32(x)), y=float(F32(y)), v=float(F32(0.5 + 0.25 * k)), phi=float(F32(-169.5 + 13.0 * k)),
                    l=float(F32(lw[0])), w=float(F32(lw[1])))

    def span(self, mode, ex, ey, axis):
        lo, hi = -45.0, 45.0
        for _, a, side, val in EE.filter_bounds(self.task, mode, ex, ey):
            if a == axis:
                lo, hi = (max(lo, float(val)), hi) if side == '>' else (lo, min(hi, float(val)))
        return lo, hi

    def inside(self, mode, ex, ey, axis):
        lo, hi = self.span(mode, ex, ey, axis)
        assert hi - lo > 4.0
        return float(F32(self.rng.uniform(lo + 1.5, hi - 1.5)))

    def inside_xy(self, mode, ex, ey):
        return self.inside(mode, ex, ey, 0), self.inside(mode, ex, ey, 1)

    def outside_xy(self, mode, ex, ey):
        bs = EE.filter_bounds(self.task, mode, ex, ey)
        x, y = self.inside_xy(mode, ex, ey)
        if not bs:
            return x, y
        _, a, side, val = bs[self.rng.integers(len(bs))]
        c = float(F32(float(val) + (-1 if side == '>' else 1) * self.rng.uniform(1.5, 5.0)))
        p = (c, y) if a == 0 else (x, c)
        assert not EE.in_range(self.task, mode, ex, ey, *p)
        return p

    def background(self, n, ex, ey, exclude=(), far=False):
        """n candidates of other modes anywhere on the map (far: none inside the collision check's 10 m box around the ego)"""
        modes = [m for m in EE.MODES12 if m not in exclude]
        out = []
        while len(out) < n:
            x, y = self.rng.uniform(-45, 45, 2)
            if far and abs(x - ex) < 12 and abs(y - ey) < 12:
                continue
            out.append(self.veh(modes[self.rng.integers(len(modes))], x, y))
        return out

    def interleave(self, a, b):
        """a and b merged at random, each keeping its own order"""
        from_a = np.zeros(len(a) + len(b), bool)
        from_a[self.rng.choice(len(a) + len(b), size=len(a), replace=False)] = True
        ia, ib = iter(a), iter(b)
        return [next(ia) if t else next(ib) for t in from_a]

    def ego_state(self, x, y, phi=90.0, vx=4.0, vy=0.05, r=0.02):
        return np.array([vx, vy, r, x, y, phi], np.float32)

    def egos(self):
        """(tag, x, y): exact and inexact float32 ego arithmetic, ego_y - 2 below / at / above -25"""
        x0, rng = LANE_X[self.task], np.random.default_rng([self.seed, 0])

        def inexact(ex, ey):
            for m in self.counts:
                for name, _, _, val in EE.filter_bounds(self.task, m, ex, ey):
                    want = {'y>ey-2': float(ey) - 2, 'x<ex+5': float(ex) + 5, 'x<ex+7': float(ex) + 7}.get(name)
                    if want is not None and want == float(val):
                        return False
            return True

        def draw(ylo, yhi):
            while True:
                ex, ey = F32(x0 + rng.uniform(-0.5, 0.5)), F32(rng.uniform(ylo, yhi))
                if inexact(ex, ey):
                    return float(ex), float(ey)
        return [('exact', x0, -30.0), ('inexact', ) + draw(-31.9, -30.1), ('at-25', float(F32(x0 + 0.25)), -23.0),
                ('inbox', ) + draw(-7.9, -6.1)]

    # ---- one scene through the reference -------------------------------------------------------------------------------------
    def params_of(self, state):
        _, params = self.env.dynamics.prediction(state[None], np.zeros((1, 2), np.float32), 10)
        params = GG.npy(params)[0].astype(np.float32)
        assert np.isfinite(params).all()
        return params

    def emit(self, label, state, rows, v_light=0, virtual=0, delta_y=None, indices=None):
        env, task = self.env, self.task
        state = np.asarray(state, np.float32)
        assert len(rows) <= M
        if indices is None:
            indices = sorted(self.rng.choice(M, size=len(rows), replace=False).tolist())       # list order = insertion order
        cand, cmode, clw = np.zeros((M, 4), np.float32), np.full((M,), EE.VACANT, np.uint8), np.zeros((M, 2), np.float32)
        for c, v in zip(indices, rows):
            cand[c] = [v['x'], v['y'], v['v'], v['phi']]
            cmode[c] = EE.MODES12.index(v['mode'])
            clw[c] = [v['l'], v['w']]
        for c in range(M):                                  # vacant rows hold a live row's record (or a spot next to the ego): mode 255 alone
            if cmode[c] == EE.VACANT:                       # must keep them out
                src = rows[self.rng.integers(len(rows))] if rows else dict(x=float(state[3]), y=float(state[4]) + 6, v=1.0, phi=90.0, l=4.8, w=2.0)
                cand[c] = [src['x'], src['y'], src['v'], src['phi']]
                clw[c] = [src['l'], src['w']]
        vehs = [dict(x=float(cand[c, 0]), y=float(cand[c, 1]), v=float(cand[c, 2]), phi=float(cand[c, 3]), l=float(clw[c, 0]),
                     w=float(clw[c, 1]), route=UTL.MODE2ROUTE[EE.MODES12[cmode[c]]]) for c in range(M) if cmode[c] != EE.VACANT]
        params = self.params_of(state)
        ego_dyn = env._get_ego_dynamics(state, params)
        env.all_vehicles, env.ego_dynamics, env.v_light = vehs, ego_dyn, int(v_light)
        env.virtual_red_light_vehicle = bool(virtual)
        best = None
        for k in range(3):                                  # the path the ego is nearest to: |delta_y| > 15 only where a scene asks for it
            env.ref_path = self.paths[k]
            o = env._get_obs()
            if best is None or abs(o[6]) < abs(best[1][6]):
                best = (k, o)
        ref_index, obs = best
        env.ref_path = self.paths[ref_index]
        assert obs.shape == (9 + 4 * self.n_slots,) and obs.dtype == np.float32
        env.obs = obs.copy()
        if delta_y is not None:
            env.obs[6] = F32(delta_y)
        tr = SimpleNamespace(n_ego_vehicles={'ego': vehs}, n_ego_dict={'ego': ego_dyn}, n_ego_collision_flag={})
        TRF.Traffic.collision_check(tr)                     # TRF:263-295
        env.traffic.collision_flag = bool(tr.n_ego_collision_flag['ego'])
        done_type, _ = env._judge_done()
        if label[0] in 'ABCD':
            # the parked form of the scene (ego v_x = v_y = r = 0, every v = 0), which the one-launch step replays: the reference's block
            # is this one with the v column cleared — the filter and the sort read neither a speed nor a heading
            env.ego_dynamics = env._get_ego_dynamics(np.array([0, 0, 0, state[3], state[4], state[5]], np.float32), params)
            env.all_vehicles = [dict(v, v=0.0) for v in vehs]
            want = obs[9:].copy()
            want[2::4] = 0
            assert np.array_equal(env._get_obs()[9:], want), label
        r = self.rec
        r['ego'].append(state); r['params'].append(params); r['cand'].append(cand); r['cand_mode'].append(cmode); r['cand_lw'].append(clw)
        r['v_light'].append(int(v_light)); r['virtual'].append(int(bool(virtual))); r['ref_index'].append(ref_index); r['obs'].append(obs)
        r['r_bound'].append(float(ego_dyn['r_bound'])); r['corners'].append(np.array(ego_dyn['Corner_point'], np.float64))
        r['done_code'].append(EE.DONE_NAMES.index(done_type)); r['collision'].append(env.traffic.collision_flag)
        r['done_delta_y'].append(F32(env.obs[6])); r['label'].append(label)
        self.k = 0
        return obs, EE.DONE_NAMES.index(done_type), ego_dyn

    def slots_of(self, obs, mode):
        at = 0
        for m, k in self.counts.items():
            if m == mode:
                return obs[9 + 4 * at: 9 + 4 * (at + k)].reshape(k, 4)
            at += k

    # ---- A: filter bounds ----------------------------------------------------------------------------------------------------
    def family_A(self):
        for tag, ex, ey in self.egos():
            for mode in self.counts:
                bounds = [(n, a, s, v) for n, a, s, v in EE.filter_bounds(self.task, mode, ex, ey)]
                if mode == 'ud':      # both candidates of max(ego_y - 2, -25), whichever of them is the bound
                    bounds += [('alt:y>ey-2', 1, '>', F32(ey) - F32(2)), ('alt:y>-25', 1, '>', F32(-25))]
                for name, axis, side, val in bounds:
                    inward = F32(np.inf) if side == '>' else F32(-np.inf)
                    for pos, c in (('on', val), ('inside', np.nextafter(val, inward)), ('outside', np.nextafter(val, -inward))):
                        other = self.inside(mode, ex, ey, 1 - axis)
                        probe = self.veh(mode, *((float(c), other) if axis == 0 else (other, float(c))))
                        rows = self.interleave([probe], self.background(6, ex, ey, exclude=(mode,)))
                        obs, _, _ = self.emit('A|%s|%s|%s|%s' % (mode, name, pos, tag), self.ego_state(ex, ey), rows)
                        if not name.startswith('alt'):      # the probe is the only candidate of its mode: in slot 0 or nowhere
                            got = self.slots_of(obs, mode)[0]
                            seen = bool(got[2] == F32(probe['v']) and got[3] == F32(probe['phi']))
                            assert seen == (pos == 'inside'), (mode, name, pos, tag)

    # ---- B: sort ties --------------------------------------------------------------------------------------------------------
    def tie_rows(self, mode, ex, ey, kind, n_before, n_group=3):
        keys = EE.sort_keys(self.task, mode)
        a1, s1 = keys[0]
        lo, hi = self.span(mode, ex, ey, a1)
        p = self.rng.uniform(lo + 10, hi - 10)
        a2 = 1 - a1
        lo2, hi2 = self.span(mode, ex, ey, a2)

        def at(c1, c2):
            return self.veh(mode, *((c1, c2) if a1 == 0 else (c2, c1)))
        before = [at(p - s1 * (1.0 + 0.7 * j), self.rng.uniform(lo2 + 1.5, hi2 - 1.5)) for j in range(n_before)]
        after = [at(p + s1 * 2.0, self.rng.uniform(lo2 + 1.5, hi2 - 1.5))]
        if kind == 'pri':      # one primary key, distinct other coordinates (the secondary key where the mode has one)
            seconds = np.sort(self.rng.uniform(lo2 + 1.5, hi2 - 1.5, n_group))
            if len(keys) > 1 and keys[1][1] < 0:
                seconds = seconds[::-1]
            group = [at(p, float(c)) for c in seconds]       # in key order where there is a secondary key
        else:                  # the same (x, y): only the insertion order is left
            c2 = self.rng.uniform(lo2 + 1.5, hi2 - 1.5)
            group = [at(p, c2) for _ in range(n_group)]
        return before, group, after

    def shuffled(self, group, others):
        """insertion order of the tie group neither its key order nor the reverse"""
        while True:
            rows = group + others
            rows = [rows[i] for i in self.rng.permutation(len(rows))]
            order = [rows.index(g) for g in group]
            if order != sorted(order) and order != sorted(order, reverse=True):
                return rows

    def family_B(self):
        es = self.egos()
        for mode, num in self.counts.items():
            keys = EE.sort_keys(self.task, mode)
            for tag, ex, ey in (es[0], es[3]):
                for kind in ('pri', 'both'):
                    for cut in (1, 2):        # how many of the group's three the slice lets in
                        if num - cut < 0:
                            continue
                        before, group, after = self.tie_rows(mode, ex, ey, kind, num - cut)
                        others = before + after + [self.veh(mode, *self.outside_xy(mode, ex, ey)) for _ in range(2)]
                        others += self.background(5, ex, ey, exclude=(mode,))
                        rows = self.shuffled(group, others)
                        obs, _, _ = self.emit('B|%s|%s|cut%d|%s' % (mode, kind, cut, tag), self.ego_state(ex, ey), rows)
                        got = self.slots_of(obs, mode)
                        if kind == 'pri' and len(keys) > 1:
                            want = group[:cut]                                   # the secondary key decides
                        else:
                            want = sorted(group, key=rows.index)[:cut]           # the insertion order decides
                        assert [(F32(w['v']), F32(w['phi'])) for w in want] == [(g[2], g[3]) for g in got[num - cut:]], (mode, kind, cut)
            # the winners are the fifth and later of the mode's candidates: four in range that sort late come first, then the winners with
            # one out of range among them
            tag, ex, ey = es[1]
            a1, s1 = keys[0]
            lo, hi = self.span(mode, ex, ey, a1)
            lo2, hi2 = self.span(mode, ex, ey, 1 - a1)
            p = self.rng.uniform(lo + 12, hi - 12)
            mk = lambda c1: self.veh(mode, *((c1, self.rng.uniform(lo2 + 1.5, hi2 - 1.5)) if a1 == 0 else (self.rng.uniform(lo2 + 1.5, hi2 - 1.5), c1)))
            late = [mk(p + s1 * (3.0 + j)) for j in range(4)]
            winners = [mk(p - s1 * (1.0 + 0.8 * j)) for j in range(num)]                      # each sorts before the one before it: the best is last
            mine = late + winners[:1] + [self.veh(mode, *self.outside_xy(mode, ex, ey))] + winners[1:]
            rows = self.interleave(mine, self.background(M - len(mine) - 3, ex, ey, exclude=(mode,)))
            obs, _, _ = self.emit('B|%s|late|%s' % (mode, tag), self.ego_state(ex, ey), rows)
            got = self.slots_of(obs, mode)
            assert [F32(w['v']) for w in winners[::-1]] == [g[2] for g in got], mode

    # ---- C: the stop-line car ------------------------------------------------------------------------------------------------
    def family_C(self):
        task, x0 = self.task, LANE_X[self.task]
        if task == 'right':                      # the car never appears (E2E:386)
            for vl, virt in ((1, 0), (0, 1), (2, 1)):
                rows = [self.veh(m, *self.inside_xy(m, x0, -30.0)) for m in self.counts] + self.background(6, x0, -30.0)
                self.emit('C|right|l%dv%d' % (vl, virt), self.ego_state(x0, -30.0), rows, vl, virt)
            return
        modes = [m for m in ('dl', 'du') if m in self.counts]
        car = dict(dl=(1.875, -22.5), du=(5.625, -22.5))
        for etag, ey in (('on', F32(-25)), ('below', EE.down(-25)), ('above', EE.up(-25))):
            for vl, virt in ((1, 0), (0, 1), (2, 1), (0, 0)):
                rows = [self.veh(m, car[m][0] + 0.25, -24.0) for m in modes] + self.background(5, x0, float(ey), exclude=modes)
                obs, _, _ = self.emit('C|line|%s|l%dv%d' % (etag, vl, virt), self.ego_state(x0, float(ey)), rows, vl, virt)
                for m in modes:
                    has = any(tuple(g) == (F32(car[m][0]), F32(-22.5), F32(0), F32(90)) for g in self.slots_of(obs, m))
                    assert has == (etag == 'below' and (vl != 0 or virt != 0) and self.counts[m] >= 2), (m, etag, vl, virt)
        ex, ey = x0, -30.0
        for m in modes:
            num, (cx, cy) = self.counts[m], car[m]
            befores = lambda k: [self.veh(m, cx, -26.0 - 0.5 * j) for j in range(k)]
            is_car = lambda g: tuple(g) == (F32(cx), F32(cy), F32(0), F32(90))
            # real cars with the stop-line car's y: a larger and a smaller x
            rows = befores(max(num - 2, 0)) + [self.veh(m, cx - 0.5, cy), self.veh(m, cx + 0.5, cy)]
            self.emit('C|tie_y|%s' % m, self.ego_state(ex, ey), self.interleave(rows, self.background(5, ex, ey, exclude=modes)), 1, 0)
            # a real car with its exact (x, y): the stop-line car was appended last, so it comes after its equal
            twin = self.veh(m, cx, cy)
            rows = befores(max(num - 2, 0)) + [twin]
            obs, _, _ = self.emit('C|tie_xy|%s' % m, self.ego_state(ex, ey), self.interleave(rows, self.background(5, ex, ey, exclude=modes)), 0, 1)
            got = self.slots_of(obs, m)
            if num >= 2:
                assert got[num - 2][2] == F32(twin['v']) and is_car(got[num - 1])
            # ... the two of them competing for the last slot: the real one takes it
            twin = self.veh(m, cx, cy)
            rows = befores(num - 1) + [twin]
            obs, _, _ = self.emit('C|last_lost|%s' % m, self.ego_state(ex, ey), self.interleave(rows, self.background(5, ex, ey, exclude=modes)), 2, 1)
            got = self.slots_of(obs, m)
            assert got[num - 1][2] == F32(twin['v']) and not any(is_car(g) for g in got)
            # ... and against a real car that sorts after it: the stop-line car takes the last slot
            rows = befores(num - 1) + [self.veh(m, cx, -20.0)]
            obs, _, _ = self.emit('C|last_won|%s' % m, self.ego_state(ex, ey), self.interleave(rows, self.background(5, ex, ey, exclude=modes)), 1, 1)
            assert is_car(self.slots_of(obs, m)[num - 1])
        if 'du' in self.counts:                  # du's own filter removes the stop-line car: ego_x + 5 <= 5.625
            edge = float(F32(float(EE.up(5.625)) - 5.0))
            assert F32(edge) + F32(5) == EE.up(5.625) and F32(EE.up(0.625)) + F32(5) == F32(5.625)
            for tag, ego_x in (('outside', 0.5), ('on', 0.625), ('on_rounded', float(EE.up(0.625))), ('inside', edge)):
                rows = self.background(6, ego_x, ey, exclude=modes)
                obs, _, _ = self.emit('C|du_x|%s' % tag, self.ego_state(ego_x, ey), rows, 1, 0)
                has = tuple(self.slots_of(obs, 'du')[0]) == (F32(5.625), F32(-22.5), F32(0), F32(90))
                assert has == (tag == 'inside'), tag

    # ---- D: counts -----------------------------------------------------------------------------------------------------------
    def family_D(self):
        es = self.egos()
        listed = list(self.counts)
        for i, (mode, num) in enumerate(self.counts.items()):
            tag, ex, ey = es[1 if i % 2 == 0 else 3]
            for name, k in (('0', 0), ('num-1', num - 1), ('num', num), ('num+1', num + 1)):
                rows = [self.veh(mode, *self.inside_xy(mode, ex, ey)) for _ in range(k)]
                rows += [self.veh(mode, *self.outside_xy(mode, ex, ey)) for _ in range(2)]
                rows = [rows[j] for j in self.rng.permutation(len(rows))]
                rows = self.interleave(rows, self.background(M - len(rows) - 4, ex, ey, exclude=(mode,)))
                self.emit('D|%s|%s' % (mode, name), self.ego_state(ex, ey), rows)
            rows = [self.veh(mode, *(self.inside_xy if j % 2 else self.outside_xy)(mode, ex, ey)) for j in range(M)]
            self.emit('D|%s|all24' % mode, self.ego_state(ex, ey), rows)
        tag, ex, ey = es[0]
        self.emit('D|none', self.ego_state(ex, ey), self.background(M, ex, ey, exclude=listed))
        rows = [self.veh(listed[j % len(listed)], *self.inside_xy(listed[j % len(listed)], ex, ey)) for j in range(M // 2)]
        self.emit('D|vacant_odd', self.ego_state(ex, ey), rows, indices=list(range(0, M, 2)))
        self.emit('D|vacant_even', self.ego_state(ex, ey), rows, indices=list(range(1, M, 2)))
        self.emit('D|empty', self.ego_state(ex, ey), [])

    # ---- E: done rules on copied quantities ------------------------------------------------------------------------------------
    def family_E(self):
        task, x0 = self.task, LANE_X[self.task]
        bounds, (gx, gy, gphi) = GOAL[task]
        for name, axis, side, val in bounds:
            inward = F32(np.inf) if side == '>' else F32(-np.inf)
            for pos, c in (('on', F32(val)), ('inside', np.nextafter(F32(val), inward)), ('outside', np.nextafter(F32(val), -inward))):
                x, y = (float(c), gy) if axis == 0 else (gx, float(c))
                self.emit('E|goal|%s|%s' % (name, pos), self.ego_state(x, y, gphi), self.background(6, x, y, far=True))
        for vl in (1, 2):
            for pos, y in (('on', F32(-25)), ('inside', EE.up(-25)), ('outside', EE.down(-25))):
                _, code, _ = self.emit('E|red|%s|l%d' % (pos, vl), self.ego_state(x0, float(y)), self.background(6, x0, float(y), far=True), vl)
                assert code == (5 if pos == 'inside' and task != 'right' else 0), (pos, vl, code)
        for sgn in (1, -1):
            for pos, d in (('on', F32(15)), ('inside', EE.up(15)), ('outside', EE.down(15))):
                _, code, _ = self.emit('E|dev|%s15|%s' % ('+' if sgn > 0 else '-', pos), self.ego_state(x0, -30.0), self.background(6, x0, -30.0, far=True),
                                       delta_y=sgn * d)
                assert code == (3 if pos == 'inside' else 0)

    # ---- F: walls ------------------------------------------------------------------------------------------------------------
    def family_F(self):
        task = self.task
        lines = sorted({(a, v) for _, a, v, _, _ in WALLS[task]})

        def clear(corners):      # float64: every corner at least d / 2 from every wall line of the task
            return all(abs((cx, cy)[a] - v) >= D_MARGIN / 2 for cx, cy in corners for a, v in lines)
        for name, axis, val, (lo, hi), inward in WALLS[task]:
            n_ok = 0
            for phi in HEADINGS:
                for _ in range(300):
                    q = int(self.rng.integers(4))
                    along = self.rng.uniform(lo, hi)
                    cxl, cyl = (2.4 if q < 2 else -2.4), (-1.0 if q & 1 else 1.0)                 # E2E:171-176
                    c, s = math.cos(math.radians(phi)), math.sin(math.radians(phi))
                    offx, offy = cxl * c - cyl * s, cxl * s + cyl * c
                    side = inward if inward else 1
                    pre = []                                  # a float64 look first: the reference's own corners decide below
                    for sgn in (1, -1):
                        w = val + sgn * side * D_MARGIN
                        tx, ty = (w, along) if axis == 0 else (along, w)
                        pre.append([UTL.judge_feasible(tx - offx + (a if i < 2 else -a) * c - b * s, ty - offy + (a if i < 2 else -a) * s + b * c, task)
                                    for i, (a, b) in enumerate(((2.4, 1.0), (2.4, -1.0), (2.4, 1.0), (2.4, -1.0)))])
                    if not all(pre[0]) or (inward and sum(pre[1]) != 3) or (not inward and not all(pre[1])):
                        continue
                    states = []
                    for sgn in (1, -1):
                        w = val + sgn * side * D_MARGIN
                        tx, ty = (w, along) if axis == 0 else (along, w)
                        states.append(self.ego_state(tx - offx, ty - offy, phi, vx=3.0, vy=0.0, r=0.0))
                    dyns = [self.env._get_ego_dynamics(st, self.params_of(st)) for st in states]
                    cs = [np.array(d['Corner_point'], np.float64) for d in dyns]
                    feas = [[UTL.judge_feasible(cx, cy, task) for cx, cy in c4] for c4 in cs]
                    near = [abs(c4[q][axis] - val) for c4 in cs]
                    if not (clear(cs[0]) and clear(cs[1]) and all(feas[0]) and all(D_MARGIN / 2 <= d <= 2 * D_MARGIN for d in near)):
                        continue      # redrawn, never kept
                    if (inward and (feas[1][q] or sum(feas[1]) != 3)) or (not inward and not all(feas[1])):
                        continue
                    for sgn, st in zip(('+d', '-d'), states):
                        bg = self.background(5, float(st[3]), float(st[4]), far=True)
                        _, code, _ = self.emit('F|%s|%s|phi%g' % (name, sgn, phi), st, bg)
                        assert (code == 2) == (bool(inward) and sgn == '-d'), (name, sgn, phi, code)
                    n_ok += 1
                    break
            assert n_ok >= 3, (task, name, n_ok)

    # ---- G: stability --------------------------------------------------------------------------------------------------------
    def family_G(self):
        x0 = LANE_X[self.task]
        for vtag, vx in (('5', 5.0), ('6.3', float(F32(6.3))), ('0', 0.0)):
            for sgn in (1, -1):
                for pos, rel in (('inside', 1 - R_MARGIN), ('outside', 1 + R_MARGIN)):
                    st = self.ego_state(x0, -30.0, vx=vx, vy=0.0, r=0.0)
                    for _ in range(4):      # r_bound depends on miu_r, which the reference derives from the state
                        rb = float(self.env._get_ego_dynamics(st, self.params_of(st))['r_bound'])
                        st[2] = F32(sgn * rb * rel)
                    rb = float(self.env._get_ego_dynamics(st, self.params_of(st))['r_bound'])
                    assert abs(abs(float(st[2])) / rb - rel) < R_MARGIN / 10, (vx, sgn, pos)
                    _, code, _ = self.emit('G|vx%s|%s|%s' % (vtag, '+' if sgn > 0 else '-', pos), st, self.background(5, x0, -30.0, far=True))
                    assert code == (0 if pos == 'inside' else 4)
        self.emit('G|vx0|r1', self.ego_state(x0, -30.0, vx=0.0, vy=0.0, r=1.0), self.background(5, x0, -30.0, far=True))

    # ---- H: the priority chain -------------------------------------------------------------------------------------------------
    def family_H(self):
        task, x0 = self.task, LANE_X[self.task]
        (gx, gy, gphi) = GOAL[task][1]
        off_goal = dict(left=(-40.0, 0.5, 180.0), straight=(0.5, 40.0, 90.0), right=(40.0, -0.5, 0.0))[task]

        def unstable(st):
            rb = float(self.env._get_ego_dynamics(st, self.params_of(st))['r_bound'])
            st[2] = F32(3.0 * rb)
            return st
        on_top = lambda st: [self.veh(list(self.counts)[0], float(st[3]) + 0.5, float(st[4]) + 0.25)]
        cases = [('col+road', self.ego_state(x0 + 3.0, -30.0), True, None, 0, 1),
                 ('road+dev', self.ego_state(x0 + 3.0, -30.0), False, 20.0, 0, 2),
                 ('dev+stab', unstable(self.ego_state(x0, -30.0)), False, -20.0, 0, 3),
                 ('stab+red', unstable(self.ego_state(x0, -10.0)), False, None, 1, 4),
                 ('red+goal', self.ego_state(gx, gy, gphi), False, None, 2, 6 if task == 'right' else 5),
                 ('all', unstable(self.ego_state(*off_goal)), True, 20.0, 1, 1)]
        for name, st, hit, dy, vl, want in cases:
            rows = (on_top(st) if hit else []) + self.background(5, float(st[3]), float(st[4]), far=True)
            _, code, _ = self.emit('H|%s' % name, st, rows, vl, delta_y=dy)
            assert code == want, (name, code)

    # ---- I: collision circles ------------------------------------------------------------------------------------------------
    def family_I(self):
        x0 = LANE_X[self.task]
        for (l, w) in LW_SET:
            l, w = float(F32(l)), float(F32(w))
            for pair in range(4):            # TRF:286-293: (front, front) (front, rear) (rear, rear) (rear, front) of (ego, vehicle)
                for pos, sgn in (('inside', -1), ('outside', 1)):
                    while True:
                        phi = float(F32(90.0 + self.rng.uniform(-25, 25)))
                        st = self.ego_state(x0 + self.rng.uniform(-0.5, 0.5), -10.0 + self.rng.uniform(-2, 2), phi)
                        ex, ey = float(st[3]), float(st[4])
                        u = np.array([math.cos(math.radians(phi)), math.sin(math.radians(phi))])
                        th = math.radians(phi) + self.rng.uniform(-0.6, 0.6)
                        dirv = np.array([math.cos(th), math.sin(th)])
                        thr = (w + 2.0) / 2 + 0.5
                        dist = thr + sgn * D_MARGIN
                        s = (l - w) / 2
                        ego_front = pair < 2
                        e_c = np.array([ex, ey]) + (1.4 if ego_front else -1.4) * u
                        v_c = e_c + (1 if ego_front else -1) * dist * dirv         # the vehicle's circle of the pair
                        same = pair in (1, 3)                                      # same heading / head to head (tail to tail)
                        vphi = float(F32(wrap180(phi if same else phi + 180.0)))
                        wv = np.array([math.cos(math.radians(vphi)), math.sin(math.radians(vphi))])
                        veh_front = pair in (0, 3)
                        p = v_c - (1 if veh_front else -1) * s * wv
                        veh = dict(mode=list(self.counts)[0], x=float(F32(p[0])), y=float(F32(p[1])), v=2.0, phi=vphi, l=l, w=w)
                        # float64 check on the float32 values the reference will see
                        ephi = float(st[5])
                        eu = np.array([math.cos(ephi / 180 * math.pi), math.sin(ephi / 180 * math.pi)])
                        vu = np.array([math.cos(veh['phi'] / 180 * math.pi), math.sin(veh['phi'] / 180 * math.pi)])
                        E = [np.array([ex, ey]) + 1.4 * eu, np.array([ex, ey]) - 1.4 * eu]
                        V = [np.array([veh['x'], veh['y']]) + s * vu, np.array([veh['x'], veh['y']]) - s * vu]
                        ds = [np.linalg.norm(E[0] - V[0]), np.linalg.norm(E[0] - V[1]), np.linalg.norm(E[1] - V[1]), np.linalg.norm(E[1] - V[0])]
                        others = [d for k, d in enumerate(ds) if k != pair]
                        if abs(ds[pair] - thr) >= D_MARGIN / 2 and (ds[pair] < thr) == (sgn < 0) and min(others) > thr + 0.25 \
                                and abs(veh['x'] - ex) < 9 and abs(veh['y'] - ey) < 9:
                            break
                    rows = self.interleave([veh], self.background(5, ex, ey, far=True))
                    _, code, _ = self.emit('I|pair%d|l%gw%g|%s' % (pair, l, w, pos), st, rows)
                    assert code == (1 if pos == 'inside' else 0), (pair, l, w, pos, code)

    def run(self, families):
        for f in families:
            self.rng = np.random.default_rng([self.seed, ord(f)])
            self.k = 0
            getattr(self, 'family_' + f)()
        r = self.rec
        dt = dict(ego=np.float32, params=np.float32, cand=np.float32, cand_mode=np.uint8, cand_lw=np.float32, v_light=np.uint8, virtual=np.uint8,
                  ref_index=np.int32, obs=np.float32, r_bound=np.float64, corners=np.float64, done_code=np.uint8, collision=np.uint8,
                  done_delta_y=np.float32)
        arrs = {k: np.array(v).astype(dt[k]) for k, v in r.items() if k != 'label'}
        arrs['label'] = np.array(r['label'])           # fixed-width unicode: loads with allow_pickle=False
        return arrs


def build(task, n_veh=None, families=None):
    """-> the arrays of g20_env_edges_<task> (n_veh None) or g20w_env_edges_<task>_N<n_veh>"""
    with widened(task, n_veh) as counts:
        b = Builder(task, counts, seed=2000 + 10 * TASKS.index(task) + (0 if n_veh is None else n_veh))
        arrs = b.run(families or (EE.FAMILIES if n_veh is None else 'ABCD'))
    if n_veh is not None:
        slots, _ = EE.tiled_counts(task, n_veh)
        arrs['obs'] = np.concatenate([arrs['obs'][:, :9], EE.regroup(arrs['obs'][:, 9:], task, n_veh)], 1)
        arrs['slot_modes'] = np.array([EE.MODES12.index(m) for m in slots], np.uint8)
    return arrs


def check(family):
    """regenerate one family of every file and compare it with the committed rows of that family"""
    for task in TASKS:
        for name, n_veh in (('g20_env_edges_%s' % task, None), ('g20w_env_edges_%s_N16' % task, 16)):
            if n_veh is not None and family not in 'ABCD':
                continue
            new, old = build(task, n_veh, families=family), np.load(os.path.join(GG.OUT, name + '.npz'), allow_pickle=False)
            rows = np.array([str(l).startswith(family + '|') for l in old['label']])
            for k, v in new.items():
                assert np.array_equal(old[k] if k == 'slot_modes' else old[k][rows], v), (name, k)
            print('reproduced %s family %s (%d scenes)' % (name, family, rows.sum()))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--check':
        return check(sys.argv[2])
    for task in TASKS:
        GG.save('g20_env_edges_%s' % task, **build(task))
        GG.save('g20w_env_edges_%s_N16' % task, **build(task, 16))


if __name__ == '__main__':
    main()
