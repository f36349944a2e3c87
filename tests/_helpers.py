"""Shared test plumbing: builds + binds the CPU oracle (oracle/envbuild_oracle.c) and wraps the
C-ABI with NumPy in/out so that the same calls can be issued against the HIP library."""
import ctypes as C
import os
import subprocess

import numpy as np

from env_build_amd import _capi, build as eb_build
from env_build_amd.endtoend_env_utils import VEHICLE_MODE_LIST, tiled_mode_list
from env_build_amd.ref_path_tables import build_ref_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
ORACLE_SO = os.path.join(ROOT, 'oracle', '_build', 'libenvbuild_oracle.so')
_oracle = None


def _oracle_source_hash():
    import hashlib
    h = hashlib.sha256()
    for f in ('oracle/envbuild_oracle.c', 'oracle/Makefile', 'include/envbuild.h'):
        with open(os.path.join(ROOT, f), 'rb') as fh:
            h.update(f.encode() + b'\0' + fh.read())
    return h.hexdigest()


def build_oracle():
    """(Re)build the checker when its sources changed — decided by content hash, not mtime, so that a library copied
    along with other sources is never reused."""
    stamp = ORACLE_SO + '.srchash'
    want = _oracle_source_hash()
    have = open(stamp).read().strip() if os.path.isfile(stamp) else None
    if not os.path.isfile(ORACLE_SO) or have != want:
        subprocess.check_call(['make', '-s', '-B', '-C', os.path.join(ROOT, 'oracle')])
        with open(stamp, 'w') as fh:
            fh.write(want + '\n')
    return ORACLE_SO


def oracle_lib():
    global _oracle
    if _oracle is None:
        build_oracle()
        _oracle = _capi.CApi(ORACLE_SO)
        assert _oracle.backend == 'oracle'
    return _oracle


def _oracle_fn(api, name, restype, argtypes):
    """a test hook the oracle exports beside the C-ABI (eb_oracle_*), typed on first use"""
    assert api.backend == 'oracle', '%s is the oracle\'s; this handle is of the %s backend' % (name, api.backend)
    fn = getattr(api.lib, name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def build_host_harness(tmp_path_factory, source, tag):
    """tests/<source> (a kernel's __host__ __device__ text behind extern "C" drivers) compiled for the host -> the loaded lib<tag>.so"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = str(tmp_path_factory.mktemp(tag) / ('lib%s.so' % tag))
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O2', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared',
                           '-I', eb_build.CSRC, os.path.join(ROOT, 'tests', source), '-o', out])
    return C.CDLL(out)


def golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


class HostModel(object):
    """One eb_handle driven with NumPy arrays.  With the oracle library the arrays are passed as
    host pointers; DeviceModel (below) stages them through torch CUDA tensors for the HIP library.
    Both issue exactly the same C-ABI calls."""

    PENALTY_ORDERS = {'reference': 0, 'record': 1}

    def __init__(self, api, task, n_veh=None, n_future=0, mode='training', modes=None, penalty_order='reference'):
        """penalty_order (the oracle only): 'reference' sums the circle-pair terms one by one, as the reference and its fixtures
        do; 'record' sums them as every HIP kernel does — the order to hold a kernel bit for bit to."""
        self.api, self.task = api, task
        native = VEHICLE_MODE_LIST[task]
        self.n_veh = len(native) if n_veh is None else int(n_veh)
        self.n_future = int(n_future)
        self.D = 6 + 3 * (self.n_future + 1) + 4 * self.n_veh
        self.T = 3 * (self.n_future + 1)
        self.h = api.create(task, self.n_veh, self.n_future,
                            _capi.MODE_TRAINING if mode == 'training' else _capi.MODE_SELECTING)
        self.paths, self.path_len_list, _ = build_ref_paths(task)
        xs = f32(np.concatenate([p[0] for p in self.paths]))
        ys = f32(np.concatenate([p[1] for p in self.paths]))
        ph = f32(np.concatenate([p[2] for p in self.paths]))
        lens = i32([len(p[0]) for p in self.paths])
        api.set_paths(self.h, _p(xs), _p(ys), _p(ph), _p(lens), 3)
        if modes is None:
            modes = native if self.n_veh == len(native) else tiled_mode_list(task, self.n_veh)
        ids = np.array([_capi.VMODE_ID[m] for m in modes], np.uint8)
        api.set_veh_modes(self.h, _p(ids), len(ids))
        self.stream = None
        self.penalty_order = 'reference'
        if penalty_order != 'reference':
            self.set_penalty_order(penalty_order)

    def set_penalty_order(self, order):
        """eb_oracle_set_penalty_order: 'reference' | 'record' (or a raw int, for the refusal test)"""
        fn = _oracle_fn(self.api, 'eb_oracle_set_penalty_order', C.c_int, [C.c_void_p, C.c_int])
        self.api.check(fn(self.h, self.PENALTY_ORDERS.get(order, order)))
        self.penalty_order = order

    def penalty_terms(self, obs):
        """eb_oracle_penalty_terms -> (t35 [n, n_veh, 4], t25 [n, n_veh, 4], road [n, 2]): the fp32 terms of the penalty sums, unsummed"""
        fn = _oracle_fn(self.api, 'eb_oracle_penalty_terms', C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4)
        ob = np.ascontiguousarray(obs, np.float32)
        n = len(ob)
        assert ob.shape == (n, self.D)
        t35, t25, road = (np.empty((n, self.n_veh, 4), np.float32), np.empty((n, self.n_veh, 4), np.float32),
                          np.empty((n, 2), np.float32))
        self.api.check(fn(self.h, n, _p(ob), _p(t35), _p(t25), _p(road)))
        return t35, t25, road

    def __del__(self):
        try:
            self.api.destroy(self.h)
        except Exception:
            pass

    # ---- staging hooks (overridden by DeviceModel) ----
    def _in(self, a, dtype=np.float32):
        return None if a is None else np.ascontiguousarray(a, dtype=dtype)

    def _out(self, shape, dtype=np.float32):
        return np.empty(shape, dtype)

    def _ptr(self, a):
        return _p(a)

    def _ret(self, a):
        return a

    # ---- one method per C-ABI entry point ----
    def f_xu(self, states, actions, tau, want_params=True):
        st, ac = self._in(states), self._in(actions)
        n = len(st)
        nxt, par = self._out((n, 6)), (self._out((n, 4)) if want_params else None)
        self.api.f_xu(self.h, n, self._ptr(st), self._ptr(ac), float(tau), self._ptr(nxt), self._ptr(par), self.stream)
        return self._ret(nxt), (self._ret(par) if want_params else None)

    def action_transform(self, actions):
        ac = self._in(actions)
        out = self._out(ac.shape)
        self.api.action_transform(self.h, len(ac), self._ptr(ac), self._ptr(out), self.stream)
        return self._ret(out)

    def compute_rewards(self, obs, actions, want_dict=True):
        ob, ac = self._in(obs), self._in(actions)
        n = len(ob)
        out5 = self._out((5, n))
        d16 = self._out((16, n)) if want_dict else None
        self.api.compute_rewards(self.h, n, self._ptr(ob), self._ptr(ac), self._ptr(out5), self._ptr(d16), self.stream)
        return self._ret(out5), (self._ret(d16) if want_dict else None)

    def compute_next_obses(self, obs, actions, ref_idx=None, path_id=0):
        ob, ac, ri = self._in(obs), self._in(actions), self._in(ref_idx, np.int32)
        out = self._out(ob.shape)
        self.api.compute_next_obses(self.h, len(ob), self._ptr(ob), self._ptr(ac), self._ptr(ri), int(path_id), self._ptr(out), self.stream)
        return self._ret(out)

    def rollout_step(self, obs, actions, ref_idx=None, path_id=0):
        ob, ac, ri = self._in(obs), self._in(actions), self._in(ref_idx, np.int32)
        n = len(ob)
        out, out5, sc = self._out(ob.shape), self._out((5, n)), self._out((n, 2))
        self.api.rollout_step(self.h, n, self._ptr(ob), self._ptr(ac), self._ptr(ri), int(path_id), self._ptr(out), self._ptr(out5), self._ptr(sc), self.stream)
        return self._ret(out), self._ret(out5), self._ret(sc)

    def rollout_step_f16(self, obs_u16, actions, ref_idx=None, path_id=0):
        """fp16 state storage (eb_rollout_step_f16): obs as uint16 bit patterns of IEEE binary16."""
        ob, ac, ri = self._in(np.ascontiguousarray(obs_u16).view(np.int16), np.int16), self._in(actions), self._in(ref_idx, np.int32)
        n = len(ob)
        out, out5, sc = self._out(ob.shape, np.int16), self._out((5, n)), self._out((n, 2))
        self.api.rollout_step_f16(self.h, n, self._ptr(ob), self._ptr(ac), self._ptr(ri), int(path_id), self._ptr(out), self._ptr(out5), self._ptr(sc), self.stream)
        return self._ret(out).view(np.uint16), self._ret(out5), self._ret(sc)

    def rollout_tape_f16(self, obs_u16, tape, ref_idx=None, path_id=0):
        ob, tp, ri = self._in(np.ascontiguousarray(obs_u16).view(np.int16), np.int16), self._in(tape), self._in(ref_idx, np.int32)
        H, n = tp.shape[0], len(ob)
        work, out, out5 = self._out(ob.shape, np.int16), self._out(ob.shape, np.int16), self._out((H, 5, n))
        self.api.rollout_tape_f16(self.h, n, H, self._ptr(ob), self._ptr(tp), self._ptr(ri), int(path_id), self._ptr(work), self._ptr(out), self._ptr(out5), self.stream)
        return self._ret(out).view(np.uint16), self._ret(out5)

    def rollout_tape(self, obs, tape, ref_idx=None, path_id=0):
        ob, tp, ri = self._in(obs), self._in(tape), self._in(ref_idx, np.int32)
        H, n = tp.shape[0], len(ob)
        work, out, out5 = self._out(ob.shape), self._out(ob.shape), self._out((H, 5, n))
        self.api.rollout_tape(self.h, n, H, self._ptr(ob), self._ptr(tp), self._ptr(ri), int(path_id), self._ptr(work), self._ptr(out), self._ptr(out5), self.stream)
        return self._ret(out), self._ret(out5)

    def gated_blocks(self, n_env):
        nb = C.c_int32()
        self.api.rollout_gated_blocks(self.h, int(n_env), C.byref(nb))
        return nb.value

    def rollout_gated(self, obs, tape, ref_idx=None, path_id=0, publish_obs=True, ready=None, spin_limit=1 << 22):
        """eb_rollout_gated with every gate already open (`ready` None) or as given -> (obs_out, out5, obs_steps, done, status)"""
        ob, tp, ri = self._in(obs), self._in(tape), self._in(ref_idx, np.int32)
        H, n = tp.shape[0], len(ob)
        work, out, out5 = self._out(ob.shape), self._out(ob.shape), self._out((H, 5, n))
        steps = self._out((H,) + tuple(ob.shape)) if publish_obs else None
        rd = self._in(np.ones(H, np.int32) if ready is None else np.asarray(ready, np.int32), np.int32)
        nb = self.gated_blocks(n)
        dn, st = self._in(np.zeros((H, max(1, nb), 16), np.int32), np.int32), self._in(np.zeros(2, np.int32), np.int32)
        self.api.rollout_gated(self.h, n, H, self._ptr(ob), self._ptr(tp), self._ptr(ri), int(path_id), self._ptr(work),
                               self._ptr(out), self._ptr(out5), self._ptr(steps), self._ptr(rd), self._ptr(dn), nb, self._ptr(st),
                               int(spin_limit), self.stream)
        return (self._ret(out), self._ret(out5), self._ret(steps) if publish_obs else None, self._ret(dn), self._ret(st))

    # ---- policy network + shield (eb_mlp_*, eb_policy_run_batch, eb_shield_is_safe) ----
    def make_mlp(self, obs_dim, n_hidden, n_units, out_dim, hidden_act, out_act, layers, obs_scale=None):
        return self.api.mlp_create_from(obs_dim, n_hidden, n_units, out_dim, hidden_act, out_act, layers, obs_scale, 0)

    def mlp_forward(self, mlp, out_dim, obs):
        ob = self._in(obs)
        out = self._out((len(ob), out_dim))
        self.api.mlp_forward(mlp, len(ob), self._ptr(ob), self._ptr(out), self.stream)
        return self._ret(out)

    def policy_run_batch(self, mlp, act_dim, obs, action_range):
        ob = self._in(obs)
        out = self._out((len(ob), act_dim))
        self.api.policy_run_batch(mlp, len(ob), self._ptr(ob), C.c_float(action_range), self._ptr(out), self.stream)
        return self._ret(out)

    def shield_is_safe(self, mlp, obs, ref_idx=None, path_id=0, steps=5, penalty=0, action_range=1.0):
        ob, ri = self._in(obs), self._in(ref_idx, np.int32)
        n = len(ob)
        a, b, act, o5 = self._out(ob.shape), self._out(ob.shape), self._out((n, 2)), self._out((5, n))
        punish, safe = self._out((n,)), self._out((n,), np.uint8)
        self.api.shield_is_safe(self.h, mlp, n, self._ptr(ob), self._ptr(ri), int(path_id), int(steps), int(penalty),
                                C.c_float(action_range), self._ptr(a), self._ptr(b), self._ptr(act), self._ptr(o5),
                                self._ptr(punish), self._ptr(safe), self.stream)
        last = a if steps % 2 == 1 else b
        return self._ret(safe), self._ret(punish), self._ret(last), self._ret(act)

    def episode_summary(self, out5_steps, obs_final):
        o5, ob = self._in(out5_steps), self._in(obs_final)
        out8 = self._out((8,))
        self.api.episode_summary(self.h, o5.shape[2], o5.shape[0], self._ptr(o5), self._ptr(ob), self._ptr(out8), self.stream)
        return self._ret(out8)

    def acc_workspace(self, n_env, horizon):
        """the workspace of an accumulating rollout of `horizon` steps over n_env envs (eb_episode_acc_bytes), filled with 0xFF:
        nothing may depend on what a rollout finds there"""
        nb = C.c_int64()
        self.api.episode_acc_bytes(self.h, int(n_env), int(horizon), C.byref(nb))
        return self._in(np.full((max(16, nb.value),), 0xFF, np.uint8), np.uint8)

    def rollout_acc(self, obs, tape, ref_idx=None, path_id=0, acc=None):
        """H x eb_rollout_step_acc (ping-ponging as eb_rollout_tape) + eb_episode_acc_finish -> (obs_out, out5 [H,5,n], summary8)"""
        ob, tp, ri = self._in(obs), self._in(tape), self._in(ref_idx, np.int32)
        H, n = tp.shape[0], len(ob)
        bufs, out5, s8 = [self._out(ob.shape), self._out(ob.shape)], self._out((H, 5, n)), self._out((8,))
        acc = self.acc_workspace(n, H) if acc is None else acc
        cur = ob
        for t in range(H):
            dst = bufs[(H - 1 - t) % 2]
            self.api.rollout_step_acc(self.h, n, self._ptr(cur), self._ptr(tp[t]), self._ptr(ri), int(path_id), self._ptr(dst),
                                      self._ptr(out5[t]), None, self._ptr(acc), t, H, self._ptr(out5[t - 1]) if t else None,
                                      self.stream)
            cur = dst
        self.api.episode_acc_finish(self.h, n, H, self._ptr(acc), self._ptr(s8), self.stream)
        return self._ret(bufs[0]), self._ret(out5), self._ret(s8)

    def plan_run(self, obs, tape, ref_idx=None, path_id=0, replays=2, with_summary=True, caller_acc=False):
        """eb_plan_create + `replays` x eb_plan_launch + destroy -> (obs_out, out5 [H,5,n], summary8).  caller_acc: the plan's
        launches accumulate into a workspace of the caller's — True: the fold is part of the plan, 'finish': the caller folds
        (summary8 == NULL, acc != NULL); False: plain launches + eb_episode_summary."""
        ob, tp, ri = self._in(obs), self._in(tape), self._in(ref_idx, np.int32)
        H, n = tp.shape[0], len(ob)
        work, out, out5 = self._out(ob.shape), self._out(ob.shape), self._out((H, 5, n))
        s8 = self._out((8,)) if with_summary else None
        acc = self.acc_workspace(n, H) if caller_acc else None
        plan = C.c_void_p()
        fold_outside = caller_acc == 'finish'       # the plan leaves the fold to the caller (summary8 == NULL, acc != NULL)
        self.api.plan_create(self.h, n, H, self._ptr(ob), self._ptr(tp), self._ptr(ri), int(path_id), self._ptr(work),
                             self._ptr(out), self._ptr(out5), None if fold_outside else self._ptr(s8), self._ptr(acc), C.byref(plan))
        try:
            for _ in range(replays):
                self.api.plan_launch(plan, self.stream)
                if fold_outside and with_summary:
                    self.api.episode_acc_finish(self.h, n, H, self._ptr(acc), self._ptr(s8), self.stream)
            res = self._ret(out), self._ret(out5), (self._ret(s8) if with_summary else None)
        finally:
            self.api.plan_destroy(plan)
        return res

    def find_closest_point(self, xs, ys, ref_idx=None, path_id=0, ratio=10):
        x, y, ri = self._in(xs), self._in(ys), self._in(ref_idx, np.int32)
        n = len(x)
        idx, pts = self._out((n,), np.int32), self._out((3, n))
        self.api.find_closest_point(self.h, n, self._ptr(x), self._ptr(y), self._ptr(ri), int(path_id), int(ratio), self._ptr(idx), self._ptr(pts), self.stream)
        return self._ret(idx), self._ret(pts)

    def path_points(self, index, n_future=0, ref_idx=None, path_id=0):
        ix, ri = self._in(index, np.int32), self._in(ref_idx, np.int32)
        n = len(ix)
        out = self._out((n_future + 1, 3, n))
        self.api.path_points(self.h, n, self._ptr(ix), self._ptr(ri), int(path_id), int(n_future), self._ptr(out), self.stream)
        return self._ret(out)

    def phi_diff(self, d):
        x = self._in(d)
        out = self._out(x.shape)
        self.api.phi_diff(self.h, x.size if hasattr(x, 'size') and not callable(x.size) else x.numel(), self._ptr(x), self._ptr(out), self.stream)
        return self._ret(out)

    def ego_predict(self, ego, actions):
        eg, ac = self._in(ego), self._in(actions)
        out = self._out((len(eg), 6))
        self.api.ego_predict(self.h, len(eg), self._ptr(eg), self._ptr(ac), self._ptr(out), self.stream)
        return self._ret(out)

    def exit_frame(self, exit_id, ego, inverse=False):
        ex, eg = self._in(exit_id, np.uint8), self._in(ego)
        out = self._out((len(eg), 6))
        self.api.exit_frame(self.h, len(eg), self._ptr(ex), int(bool(inverse)), self._ptr(eg), self._ptr(out), self.stream)
        return self._ret(out)

    def env_reset(self, n_env, seed, counter, training, ego, params, ref_idx, mask=None, episode_step=None):
        """-> (ego, params, ref_idx, virtual_next, done_code[, episode_step]) after eb_env_reset on copies of the given state"""
        eg, pr, ri = self._in(np.array(ego, np.float32)), self._in(np.array(params, np.float32)), self._in(np.array(ref_idx, np.int32), np.int32)
        mk = self._in(mask, np.uint8)
        vn, dc = self._out((n_env,), np.uint8), self._out((n_env,), np.uint8)
        es = None if episode_step is None else self._in(np.array(episode_step, np.int32), np.int32)
        for t in (vn, dc):
            t[...] = 7
        self.api.env_reset(self.h, n_env, self._ptr(mk), C.c_uint64(seed), C.c_uint64(counter), int(training), self._ptr(eg),
                           self._ptr(pr), self._ptr(ri), self._ptr(vn), self._ptr(dc), self._ptr(es), self.stream)
        res = self._ret(eg), self._ret(pr), self._ret(ri), self._ret(vn), self._ret(dc)
        return res if es is None else res + (self._ret(es),)

    def ego_dynamics(self, ego, params):
        """eb_ego_dynamics -> [n, 11] = alpha_f_bound, alpha_r_bound, r_bound, 4 corner points (x, y)"""
        eg, pr = self._in(ego), self._in(params)
        out = self._out((len(eg), 11))
        self.api.ego_dynamics(self.h, len(eg), self._ptr(eg), self._ptr(pr), self._ptr(out), self.stream)
        return self._ret(out)

    def env_reset_pool(self, traffic, seed, counter, training, ego, params, ref_idx, virtual, v_light, cand, cand_mode, obs, pool,
                       mask=None, obs_src=None, done_src=None, episode_step=None):
        """eb_env_reset_pool on copies of the state -> (ego, params, ref_idx, virtual, v_light, done_code, cand, obs[, episode_step])"""
        cp = lambda a, t: self._in(np.array(a, t))          # in/out arguments: explicit copies (the oracle writes in place)
        eg, pr, ri = cp(ego, np.float32), cp(params, np.float32), self._in(np.array(ref_idx, np.int32), np.int32)
        vf, vl, mk = self._in(np.array(virtual, np.uint8), np.uint8), self._in(np.array(v_light, np.uint8), np.uint8), self._in(mask, np.uint8)
        cd, cm, ob = cp(cand, np.float32), self._in(cand_mode, np.uint8), cp(obs, np.float32)
        n, m = len(eg), cd.shape[1]
        dc = self._out((n,), np.uint8)
        dc[...] = 7
        en = self._in(pool['entry'])
        osrc, dsrc = self._in(obs_src), self._in(done_src, np.uint8)
        rs = _capi.EbRespawn(self._ptr(en).value, 0.0, float(pool['span']), float(pool['v_max']), int(pool['seed']), int(pool['counter']),
                             float(pool['edge_span']))
        es = None if episode_step is None else self._in(np.array(episode_step, np.int32), np.int32)
        self.api.env_reset_pool(self.h, traffic.h, n, self._ptr(mk), C.c_uint64(seed), C.c_uint64(counter), int(training), self._ptr(eg),
                                self._ptr(pr), self._ptr(ri), self._ptr(vf), self._ptr(vl), self._ptr(dc), self._ptr(es), m, self._ptr(cd),
                                self._ptr(cm), C.byref(rs), self._ptr(ob), self._ptr(osrc), self._ptr(dsrc), self.stream)
        return [self._ret(x) for x in (eg, pr, ri, vf, vl, dc, cd, ob) + (() if es is None else (es,))]

    def tracking_error(self, xs, ys, phis, vs, n_future, ref_idx=None, path_id=0):
        x, y, ph, v, ri = self._in(xs), self._in(ys), self._in(phis), self._in(vs), self._in(ref_idx, np.int32)
        n = len(x)
        out = self._out((n, 3 * (n_future + 1)))
        self.api.tracking_error(self.h, n, self._ptr(x), self._ptr(y), self._ptr(ph), self._ptr(v), self._ptr(ri), int(path_id), int(n_future), self._ptr(out), self.stream)
        return self._ret(out)

    def veh_predict(self, veh):
        v = self._in(veh)
        out = self._out(v.shape)
        self.api.veh_predict(self.h, len(v), self._ptr(v), self._ptr(out), self.stream)
        return self._ret(out)

    def ss(self, obs, actions, ref_idx=None, path_id=0, lam=0.1):
        ob, ac, ri = self._in(obs), self._in(actions), self._in(ref_idx, np.int32)
        out = self._out((len(ob),))
        self.api.ss(self.h, len(ob), self._ptr(ob), self._ptr(ac), self._ptr(ri), int(path_id), float(lam), self._ptr(out), self.stream)
        return self._ret(out)

    def env_ego_step(self, ego, actions):
        eg, ac = self._in(ego), self._in(actions)
        n = len(eg)
        nxt, par = self._out((n, 6)), self._out((n, 4))
        self.api.env_ego_step(self.h, n, self._ptr(eg), self._ptr(ac), self._ptr(nxt), self._ptr(par), self.stream)
        return self._ret(nxt), self._ret(par)

    def _shifted(self, a):
        """the float32 array at an address 4 bytes past a 16-byte boundary (the one-launch kernels want their arrays aligned: a
        library call with such an argument takes its separate-launch path)"""
        a = np.ascontiguousarray(a, np.float32)
        buf = np.empty(a.size + 8, np.float32)
        k = ((4 - buf.ctypes.data) % 16) // 4
        v = buf[k:k + a.size].reshape(a.shape)
        v[...] = a
        return v

    def get_obs(self, ego, cand, cand_mode, v_light=None, ref_idx=None, path_id=0, virtual=None, exit_id=None, row_mask=None,
                obs_init=None, shift=()):
        """shift: which of 'ego', 'cand' to hand over 4 bytes off a 16-byte boundary (see _shifted)"""
        eg, cd, ri = self._in(ego), self._in(cand), self._in(ref_idx, np.int32)
        if 'ego' in shift:
            eg = self._shifted(ego)
        if 'cand' in shift:
            cd = self._shifted(cand)
        cm, vl, vf, ex = self._in(cand_mode, np.uint8), self._in(v_light, np.uint8), self._in(virtual, np.uint8), self._in(exit_id, np.uint8)
        n, m = len(eg), cd.shape[1]
        out = self._out((n, self.D)) if obs_init is None else self._in(np.array(obs_init, np.float32))   # (a copy: the oracle writes in place)
        rm = self._in(row_mask, np.uint8)
        self.api.get_obs(self.h, n, self._ptr(eg), self._ptr(ri), int(path_id), m, self._ptr(cd), self._ptr(cm), self._ptr(vl),
                         self._ptr(vf), self._ptr(ex), self._ptr(rm), self._ptr(out), self.stream)
        return self._ret(out)

    def env_step(self, traffic, obs, raw, ego, cand, cand_mode, ref_idx=None, path_id=0, cand_lw=None, v_light=None,
                 virtual=None, respawn=None, want_scaled=True, want_dict=True, scale_in_place=False, auto_reset=None, flow=None,
                 time_limit=None):
        """eb_env_step on copies of the state -> (scaled, out5, d16, ego, params, cand, obs_out, done_code).
        scale_in_place: the scaled actions overwrite the (copy of the) raw action array.
        respawn: dict(entry [M, 5], limit, span, v_max, seed, counter) — the pool's re-entry as the step's last stage.
        auto_reset: dict(seed, counter, training, pool=dict(entry, span, v_max, seed, counter, edge_span), final_obs=bool) — the
        envs the step finishes are reset in the same call (ABI 4); the result gains (ref_idx, virtual, v_light, final_obs),
        final_obs pre-filled with NaN.
        time_limit: (episode_step [B] int32, max_episode_steps) — ABI 5; the result gains the step counts after the call (last)."""
        B, M = len(ego), cand.shape[1]
        e_io, c_io = self._in(np.array(ego, np.float32)), self._in(np.array(cand, np.float32))
        ob, rw, ri = self._in(obs), self._in(raw), self._in(ref_idx, np.int32)
        cm, lw = self._in(cand_mode, np.uint8), self._in(cand_lw)
        vl, vf = self._in(v_light, np.uint8), self._in(virtual, np.uint8)
        par, out5 = self._out((B, 4)), self._out((5, B))
        sc = rw if scale_in_place else (self._out((B, 2)) if want_scaled else None)
        dd = self._out((16, B)) if want_dict else None
        obs_o, code = self._out(np.asarray(obs).shape), self._out((B,), np.uint8)
        rs, entry = None, None
        if respawn is not None:
            entry = self._in(respawn['entry'])
            rs = _capi.EbRespawn(self._ptr(entry).value, float(respawn['limit']),
                                 float(respawn['span']), float(respawn['v_max']), int(respawn['seed']), int(respawn['counter']))
        ar, fl, extra = None, None, ()
        vp = lambda t: None if t is None else self._ptr(t).value
        if auto_reset is not None or flow is not None:      # the arrays the call rewrites: explicit copies, shared by the two structs
            vl = None if v_light is None else self._in(np.array(v_light, np.uint8), np.uint8)
        if auto_reset is not None:
            pool = auto_reset.get('pool')
            pentry = None if pool is None else self._in(pool['entry'])
            ri = None if ref_idx is None else self._in(np.array(ref_idx, np.int32), np.int32)
            vf = self._in(np.array(virtual, np.uint8), np.uint8)
            fo = self._in(np.full(np.asarray(obs).shape, np.nan, np.float32)) if auto_reset.get('final_obs', True) else None
            pr = _capi.EbRespawn() if pool is None else _capi.EbRespawn(self._ptr(pentry).value, 0.0, float(pool['span']), float(pool['v_max']),
                                                                        int(pool['seed']), int(pool['counter']), float(pool['edge_span']))
            ar = _capi.EbAutoReset(int(auto_reset['seed']), int(auto_reset['counter']), int(auto_reset['training']), vp(ri), vp(vf),
                                   vp(vl), pr, vp(fo))
            fr_extra = ()
            if 'flow' in auto_reset:       # ABI 5: the flow source's part of reset — dict(cand_len [M], phase0 [B], random_phase, seed, counter)
                fr = auto_reset['flow']
                f_len, f_ph = self._in(fr['cand_len']), self._in(np.array(fr['phase0'], np.uint8), np.uint8)
                ar.flow_cand_len, ar.flow_phase0, ar.flow_random_phase = vp(f_len), vp(f_ph), int(fr['random_phase'])
                ar.flow_seed, ar.flow_counter = int(fr['seed']), int(fr['counter'])
                fr_extra = (f_ph,)
            for k in ('ref_idx', 'virtual', 'v_light'):                  # test hook: a pointer that is NOT the call's argument
                if k in auto_reset.get('wrong', ()):
                    setattr(ar, {'virtual': 'virtual_flag'}.get(k, k), vp(self._out((B,), np.int32 if k == 'ref_idx' else np.uint8)))
            extra = (ri, vf, vl, fo) + fr_extra
        if flow is not None:
            # flow: dict(per_route, active, timer, emitted, sim_step, lane, period, v_max, dt, exit_range, accel, lane_len, light_cycle,
            # seed, counter) — eb_traffic_flow_step as the call's last stage; the result gains (active, timer, emitted, sim_step,
            # cand_mode, v_light) after it
            cm = self._in(np.array(cand_mode, np.uint8), np.uint8)          # (a copy: the call rewrites it)
            f_act, f_tim = self._in(np.array(flow['active'], np.uint8), np.uint8), self._in(np.array(flow['timer'], np.float32))
            f_emi, f_sim = self._in(np.array(flow['emitted'], np.int32), np.int32), self._in(np.array(flow['sim_step'], np.int32), np.int32)
            f_lane, f_per, f_vm = self._in(flow['lane']), self._in(flow['period']), self._in(flow['v_max'])
            fl = _capi.EbFlowRule(int(flow['per_route']), vp(f_act), vp(f_tim), vp(f_emi), vp(f_sim), vp(f_lane), vp(f_per), vp(f_vm),
                                  float(flow['dt']), float(flow['exit_range']), float(flow['accel']), float(flow['lane_len']),
                                  int(flow['light_cycle']), int(flow['seed']), int(flow['counter']),
                                  vp(self._out((B, M), np.uint8)) if 'mode' in flow.get('wrong', ()) else vp(cm),
                                  vp(self._out((B,), np.uint8)) if 'v_light' in flow.get('wrong', ()) else vp(vl))
            extra = extra + (f_act, f_tim, f_emi, f_sim, cm, vl)
        tl = None
        if time_limit is not None:
            es = self._in(np.array(time_limit[0], np.int32), np.int32)
            tl = _capi.EbTimeLimit(self._ptr(es).value, int(time_limit[1]))
            extra = extra + (es,)
        self.api.env_step(self.h, traffic.h, B, self._ptr(ob), self._ptr(rw), self._ptr(ri), int(path_id), self._ptr(e_io),
                          self._ptr(par), M, self._ptr(c_io), self._ptr(cm), self._ptr(lw), self._ptr(vl), self._ptr(vf),
                          self._ptr(sc), self._ptr(out5), self._ptr(dd), self._ptr(obs_o), self._ptr(code),
                          C.byref(rs) if rs is not None else None, C.byref(ar) if ar is not None else None,
                          C.byref(fl) if fl is not None else None, C.byref(tl) if tl is not None else None, self.stream)
        return [None if x is None else self._ret(x) for x in (sc, out5, dd, e_io, par, c_io, obs_o, code) + extra]

    def traffic_respawn(self, cand, entry, limit, span, v_max, seed, counter, mask=None, ego=None, edge_span=0.0):
        """eb_traffic_respawn on a copy of the candidates -> (cand, respawned)"""
        cd, en, mk, eg = self._in(np.array(cand, np.float32)), self._in(entry), self._in(mask, np.uint8), self._in(ego)
        B, M = cd.shape[0], cd.shape[1]
        flags = self._out((B, M), np.uint8)
        self.api.traffic_respawn(self.h, B, M, self._ptr(cd), self._ptr(en), C.c_float(limit), C.c_float(span), C.c_float(v_max),
                                 C.c_uint64(seed), C.c_uint64(counter), self._ptr(mk), self._ptr(flags), self._ptr(eg), C.c_float(edge_span), self.stream)
        return self._ret(cd), self._ret(flags)

    def traffic_flow_reset(self, K, mask, ego, cand, active, timer, emitted, sim_step, phase0, lane, period, v_max, cand_len, lane_len,
                           random_phase, training, seed, counter, cand_mode, v_light):
        """eb_traffic_flow_reset on copies of the state -> (cand, active, timer, emitted, sim_step, phase0, cand_mode, v_light)"""
        cp = lambda a, t, tt=None: self._in(np.array(a, t), tt or t)
        cd, ac, tm = cp(cand, np.float32), cp(active, np.uint8), cp(timer, np.float32)
        em, ss, ph = cp(emitted, np.int32), cp(sim_step, np.int32), cp(phase0, np.uint8)
        md, vl = cp(cand_mode, np.uint8), cp(v_light, np.uint8)
        mk, eg = self._in(mask, np.uint8), self._in(ego)
        ln, pe, vm, cl = self._in(lane), self._in(period), self._in(v_max), self._in(cand_len)
        B = cd.shape[0]
        self.api.traffic_flow_reset(self.h, B, int(K), self._ptr(mk), self._ptr(eg), self._ptr(cd), self._ptr(ac), self._ptr(tm), self._ptr(em),
                                    self._ptr(ss), self._ptr(ph), self._ptr(ln), self._ptr(pe), self._ptr(vm), self._ptr(cl), C.c_float(lane_len),
                                    int(random_phase), int(training), C.c_uint64(seed), C.c_uint64(counter), self._ptr(md), self._ptr(vl),
                                    self.stream)
        return [self._ret(x) for x in (cd, ac, tm, em, ss, ph, md, vl)]

    def traffic_flow_step(self, K, cand, active, timer, emitted, sim_step, lane, period, v_max, dt, exit_range, accel, lane_len,
                          light_cycle, seed, counter, v_light):
        """eb_traffic_flow_step on copies of the state -> (cand, active, timer, emitted, sim_step, cand_mode, v_light)"""
        cd, ac = self._in(np.array(cand, np.float32)), self._in(np.array(active, np.uint8), np.uint8)
        tm, em = self._in(np.array(timer, np.float32)), self._in(np.array(emitted, np.int32), np.int32)
        ss, vl = self._in(np.array(sim_step, np.int32), np.int32), self._in(np.array(v_light, np.uint8), np.uint8)
        ln, pe, vm = self._in(lane), self._in(period), self._in(v_max)
        B, M = cd.shape[0], cd.shape[1]
        md = self._out((B, M), np.uint8)
        self.api.traffic_flow_step(self.h, B, int(K), self._ptr(cd), self._ptr(ac), self._ptr(tm), self._ptr(em), self._ptr(ss), self._ptr(ln),
                                   self._ptr(pe), self._ptr(vm), C.c_float(dt), C.c_float(exit_range), C.c_float(accel), C.c_float(lane_len),
                                   int(light_cycle), C.c_uint64(seed), C.c_uint64(counter), self._ptr(md), self._ptr(vl), self.stream)
        return [self._ret(x) for x in (cd, ac, tm, em, ss, md, vl)]

    def judge_done(self, ego, params, obs, cand, cand_mode, cand_lw, v_light):
        eg, pr, ob, cd = self._in(ego), self._in(params), self._in(obs), self._in(cand)
        lw, cm, vl = self._in(cand_lw), self._in(cand_mode, np.uint8), self._in(v_light, np.uint8)
        n, m = len(eg), cd.shape[1]
        out = self._out((n,), np.uint8)
        self.api.judge_done(self.h, n, self._ptr(eg), self._ptr(pr), self._ptr(ob), m, self._ptr(cd), self._ptr(cm), self._ptr(lw), self._ptr(vl), self._ptr(out), self.stream)
        return self._ret(out)


class DeviceModel(HostModel):
    """Same calls against libenvbuild_hip.so: inputs are copied to cuda:0 with torch (plumbing
    only), outputs allocated there, results copied back for comparison."""

    def __init__(self, task, **kw):
        import torch
        self.torch = torch
        self.dev = torch.device('cuda', 0)
        HostModel.__init__(self, _capi.hip_api(), task, **kw)
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if DeviceModel.ENV_WAVES:
            self.api.debug_set_env_waves(self.h, DeviceModel.ENV_WAVES)

    def set_tape_stepwise(self, on):
        """eb_rollout_tape as H per-step launches (True) or one tape-kernel launch (False, the default)."""
        self.api.debug_set_tape_stepwise(self.h, int(bool(on)))

    def set_tile(self, variant):
        """Force the rollout kernel's tile shape (eb_debug_set_tile; -1 = pick by batch size)."""
        self.api.debug_set_tile(self.h, int(variant))

    def set_env_waves(self, waves):
        """Force the waves per block of the one-launch env kernels (eb_debug_set_env_waves; 4 / 8, 0 = by grid size)."""
        self.api.debug_set_env_waves(self.h, int(waves))

    def rollout_plan(self, n_env):
        """eb_debug_rollout_plan -> (tile shape 0 / 1 / 2, workgroups, rolling loads, priority by progress) for a batch of n_env"""
        out = (C.c_int32 * 4)()
        self.api.debug_rollout_plan(self.h, int(n_env), out)
        return tuple(out)

    def set_rollout_sched(self, rolling=-1, by_progress=-1):
        """eb_debug_set_rollout_sched: the per-step kernel's rolling record loads / issue priority by progress (-1 = by grid size)."""
        self.api.debug_set_rollout_sched(self.h, int(rolling), int(by_progress))

    ENV_WAVES = 0     # eb_debug_set_env_waves for every DeviceModel made from now on (scripts/fuzz_env_auto.py --waves)

    _TD = {np.dtype(np.float32): 'float32', np.dtype(np.int32): 'int32', np.dtype(np.uint8): 'uint8',
           np.dtype(np.int16): 'int16'}

    def _in(self, a, dtype=np.float32):
        if a is None:
            return None
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def _out(self, shape, dtype=np.float32):
        return self.torch.empty(tuple(shape), dtype=getattr(self.torch, self._TD[np.dtype(dtype)]), device=self.dev)

    def _shifted(self, a):
        t = self._in(a)
        buf = self.torch.empty(t.numel() + 8, dtype=self.torch.float32, device=self.dev)
        k = ((4 - buf.data_ptr()) % 16) // 4
        v = buf[k:k + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    def _ptr(self, t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _ret(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy()


PARITY_LOG = {}   # check name -> (largest excess over rtol seen, the atol it was held to); printed by conftest at the end


def close(got, want, rtol, atol, what):
    """|got - want| <= rtol * |want| + atol elementwise, reporting the OBSERVED excess over the rtol term (what the atol
    has to absorb) — so that a tolerance wider than the data needs is visible in the test output."""
    a, b = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert a.shape == b.shape, '%s: shape %s vs %s' % (what, a.shape, b.shape)
    ex = float(np.max(np.abs(a - b) - rtol * np.abs(b))) if a.size else 0.0
    old = PARITY_LOG.get(what, (-np.inf, atol))
    PARITY_LOG[what] = (max(old[0], ex), atol)
    assert ex <= atol, '%s: max excess over rtol %.0e is %.3e > atol %.1e' % (what, rtol, ex, atol)
    return ex


def max_err(a, b, rtol):
    """max over elements of |a-b| - rtol*|b| (<= atol passes)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) - rtol * np.abs(b))) if a.size else 0.0


# ---- the rollout kernels against the oracle: the start rows and the bars (tests/test_gpu_parity.py, test_gpu_gated.py,
#      test_gpu_kernel_census.py) ----
# PEN_RTOL is what a penalty sum is held to where the expected side sums the circle-pair terms in ANOTHER order than the kernels
# (DESIGN.md section 4).  Against the oracle with penalty_order='record' nothing needs it: check_out5(..., exact=True).  It still
# applies to: the derived checks of reference fixtures (their order is the reference's), __graft_entry__.smoke(), and the scripts
# under scripts/fuzz_* (whose host models sum in the reference's order; they may move to exact=True as well).
PEN_RTOL = 1e-6


def record_host(task, **kw):
    """the oracle whose penalty sums are associated as every HIP kernel's are: the expected side of check_out5(..., exact=True)"""
    return HostModel(oracle_lib(), task, penalty_order='record', **kw)


def initial_obs(host, inp):
    """make_rollout_inputs' scene as observation rows, the tracking columns from the oracle"""
    from env_build_amd.synthetic import assemble_obs
    ego = inp['ego']
    trk = host.tracking_error(ego[:, 3], ego[:, 4], ego[:, 5], ego[:, 0], host.n_future, ref_idx=inp['ref_idx'])
    return assemble_obs(ego, trk, inp['veh'])


def bits_equal(got, want, what):
    """np.array_equal, except that where `want` is NaN `got` must be NaN too (any NaN: its payload is nobody's contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: shape %s vs %s' % (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN in other places' % what
    bad = np.argwhere(~nan & (got != want))
    assert not len(bad), '%s: %d of %d differ, first at %s: got %r, want %r' % (
        what, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def check_out5(o5_d, o5_h, where, exact=False):
    """rewards and veh2road4real bit for bit; the three penalty sums within PEN_RTOL, or — exact=True, the expected side an
    oracle with penalty_order='record' — bit for bit as well"""
    if exact:
        for k in range(5):
            bits_equal(o5_d[k], o5_h[k], 'out5[%d] %s' % (k, where))
        return
    assert np.array_equal(o5_d[0], o5_h[0]), 'rewards differ %s' % where
    assert np.array_equal(o5_d[4], o5_h[4]), 'veh2road4real differs %s' % where
    for k in (1, 2, 3):
        np.testing.assert_allclose(o5_d[k], o5_h[k], rtol=PEN_RTOL, atol=0, err_msg='out5[%d] %s' % (k, where))


def stepwise(host, obs0, inp, H):
    """H x rollout_step -> (last obs, out5 [H, 5, n], obs of every step [H, n, D])"""
    obs, o5s, states = obs0, [], []
    for t in range(H):
        obs, o5, _ = host.rollout_step(obs, inp['actions'][t], inp['ref_idx'])
        o5s.append(o5); states.append(obs)
    return obs, np.stack(o5s), np.stack(states)


def check_out5_steps(o5_d, o5_h, exact=False):
    """check_out5's rule over [H, 5, n]"""
    if exact:
        bits_equal(o5_d, o5_h, 'out5 of every step')
        return
    assert np.array_equal(o5_d[:, 0], o5_h[:, 0]) and np.array_equal(o5_d[:, 4], o5_h[:, 4])
    np.testing.assert_allclose(o5_d, o5_h, rtol=1e-6, atol=0)
