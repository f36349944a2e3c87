"""The harness of the one-launch tape families (eb_rollout_tape_vjp, _cand, _cand_vjp, _sample, _ilqr): the device model with every
t_* entry, the synthetic and edge scenes, the candidate tapes, the bit comparisons, the G17 solver setup, the example loader and the
bound helpers the host and GPU iLQR tests share.  A helper module like _helpers.py and _grad_cases.py: pytest does not collect it, and
importing it touches no device (torch is imported inside the functions that need it)."""
import ctypes as C
import glob
import importlib.util
import os

import numpy as np

from env_build_amd.synthetic import make_rollout_inputs, assemble_obs
from tests._helpers import GOLDEN, ROOT, DeviceModel, golden
from tests._grad_cases import NEAR_R

NATIVE = {'left': 8, 'straight': 9, 'right': 5}
# weights of `cost`: zeros in different rows, and all zero.  Every set weighs the reward row (<= 0: minus sums of squares, DAM:198-207)
# negatively and the penalty rows (>= 0: squared overlaps, DAM:218-295) positively, as every cost of this project does
# (mpc.DEFAULT_WEIGHTS, examples/adp_policy_gradient.py): the terms of J then share one sign, and the bound on the difference between
# two summation orders — relative to |J| — means what it says; weights that let the terms cancel would test the bound's form, not
# the kernel.
WEIGHTS = ((-1.0, 10.0, 0.0, 0.0, 0.0), (0.0, 0.0, 2.0, 0.0, 1.0), (-0.5, 0.0, 0.0, 0.25, 0.0), (-1.0, 10.0, 0.5, 0.25, 2.0),
           (0.0, 0.0, 0.0, 0.0, 0.0))
G5 = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, 'g5_rollout_*.npz')))
ILQR_OUT = ('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv', 'cand', 'lq')      # eb_rollout_tape_ilqr's outputs, in its argument order


def _floats(v):
    return None if v is None else (C.c_float * len(v))(*[float(x) for x in v])


def _path_ids(v):
    return None if v is None else C.cast((C.c_int32 * len(v))(*[int(x) for x in v]), C.c_void_p)


class TapeModel(DeviceModel):
    """DeviceModel + the tape entries of include/envbuild_grad.h, envbuild_cand.h, envbuild_cand_grad.h, envbuild_sample.h and
    envbuild_ilqr.h; the t_* methods take and return torch tensors on the device"""

    def __init__(self, task, **kw):
        self.mode = kw.get('mode', 'training')
        DeviceModel.__init__(self, task, **kw)

    def to_dev(self, a, dtype=np.float32):
        return self._in(a, dtype)

    def _limits(self, entry, *args, n=1):
        """the n int32 limits an eb_rollout_tape_*_max entry reports for (*args)"""
        out = [C.c_int32(0) for _ in range(n)]
        getattr(self.api, entry)(self.h, *args, *[C.byref(v) for v in out])
        return tuple(v.value for v in out)

    # ---- include/envbuild_grad.h ----
    def t_tape_vjp(self, obs0, tape, ri, path_id, g_final=None, g5=None, w5=None, out5=True, obs_out=True, g_obs0=True, g_tape=True):
        torch = self.torch
        H, n, nd = tape.shape[0], obs0.shape[0], self.D - 4 * self.n_veh
        mk = lambda want, shape: torch.full(shape, float('nan'), device=self.dev) if want else None
        o5, oo, g0, gt = mk(out5, (H, 5, n)), mk(obs_out, (n, self.D)), mk(g_obs0, (n, nd)), mk(g_tape, (H, n, 2))
        self.api.rollout_tape_vjp(self.h, n, H, self._ptr(obs0), self._ptr(tape), self._ptr(ri), int(path_id), self._ptr(g_final),
                                  0 if g_final is None else g_final.shape[1], self._ptr(g5), _floats(w5), self._ptr(o5), self._ptr(oo),
                                  self._ptr(g0), self._ptr(gt), self.stream)
        return o5, oo, g0, gt

    def t_step_vjp(self, obs, actions, ri, path_id, g_obs_out, g_out5):
        """eb_rollout_step_vjp, ld_in == nd -> g_obs_in [n, nd], g_actions [n, 2]"""
        n, nd = obs.shape[0], self.D - 4 * self.n_veh
        gi, ga = self.torch.full((n, nd), float('nan'), device=self.dev), self.torch.full((n, 2), float('nan'), device=self.dev)
        self.api.rollout_step_vjp(self.h, n, self._ptr(obs), self._ptr(actions), self._ptr(ri), int(path_id), self._ptr(g_obs_out),
                                  g_obs_out.shape[1], self._ptr(g_out5), self._ptr(gi), nd, self._ptr(ga), self.stream)
        return gi, ga

    def t_composed(self, obs0, tape, ri, path_id, g_final=None, g5=None):
        """what a user had to do before: H eb_rollout_step launches that keep every pre-step obs, then eb_rollout_chain_vjp"""
        torch = self.torch
        H, n, nd = tape.shape[0], obs0.shape[0], self.D - 4 * self.n_veh
        steps = torch.empty((H + 1, n, self.D), device=obs0.device)
        steps[0] = obs0
        o5, sc = torch.empty((H, 5, n), device=obs0.device), torch.empty((n, 2), device=obs0.device)
        for t in range(H):
            self.api.rollout_step(self.h, n, self._ptr(steps[t]), self._ptr(tape[t]), self._ptr(ri), int(path_id), self._ptr(steps[t + 1]),
                                  self._ptr(o5[t]), self._ptr(sc), self.stream)
        work, g0 = torch.empty((n, nd), device=obs0.device), torch.empty((n, nd), device=obs0.device)
        gt = torch.empty((H, n, 2), device=obs0.device)
        self.api.rollout_chain_vjp(self.h, n, H, self._ptr(steps), self._ptr(tape), self._ptr(ri), int(path_id), self._ptr(g_final),
                                   0 if g_final is None else g_final.shape[1], self._ptr(g5), self._ptr(work), self._ptr(g0),
                                   self._ptr(gt), self.stream)
        return o5, steps[H], g0, gt

    def t_forward_tape(self, obs0, tape, ri, path_id):
        torch = self.torch
        H, n = tape.shape[0], obs0.shape[0]
        work, out, o5 = torch.empty_like(obs0), torch.empty_like(obs0), torch.empty((H, 5, n), device=obs0.device)
        self.api.rollout_tape(self.h, n, H, self._ptr(obs0), self._ptr(tape), self._ptr(ri), int(path_id), self._ptr(work), self._ptr(out),
                              self._ptr(o5), self.stream)
        return o5, out

    def max_horizon(self):
        return self._limits('rollout_tape_vjp_max_horizon')[0]

    # ---- include/envbuild_cand.h ----
    def cand_max(self, horizon=25):
        return self._limits('rollout_tape_cand_max', int(horizon))[0]

    def t_cand(self, obs0, tapes, ri=None, ref_ld=0, path_ids=None, path_id=1, retrack=False, w5=None, out5=True, cost=None):
        torch = self.torch
        K, H, n = tapes.shape[0], tapes.shape[1], obs0.shape[0]
        cost = (w5 is not None) if cost is None else cost
        o5 = torch.full((K, H, 5, n), float('nan'), device=self.dev) if out5 else None
        J = torch.full((K, n), float('nan'), device=self.dev) if cost else None
        self.api.rollout_tape_cand(self.h, n, K, H, self._ptr(obs0), self._ptr(tapes), self._ptr(ri), int(ref_ld), _path_ids(path_ids),
                                   int(path_id), int(bool(retrack)), _floats(w5), self._ptr(o5), self._ptr(J), self.stream)
        return o5, J

    def cand_cost(self, obs0, tapes, ri, pid, w5):
        """eb_rollout_tape_cand's cost [K, n] of the tapes [K, H, n, 2], in chunks of its limit"""
        limit = self.cand_max(tapes.shape[1])
        return self.torch.cat([self.t_cand(obs0, tapes[k:k + limit].contiguous(), ri, 0, None, pid, False, w5, out5=False)[1]
                               for k in range(0, tapes.shape[0], limit)])

    # ---- include/envbuild_cand_grad.h ----
    def cand_grad_max(self, horizon=25):
        return self._limits('rollout_tape_cand_vjp_max', int(horizon))[0]

    def t_cand_vjp(self, obs0, tapes, ri=None, ref_ld=0, path_ids=None, path_id=1, retrack=False, w5=WEIGHTS[0], out5=True, cost=True,
                   g_obs0=True, g_tapes=True):
        torch = self.torch
        K, H, n, nd = tapes.shape[0], tapes.shape[1], obs0.shape[0], self.D - 4 * self.n_veh
        mk = lambda want, shape: torch.full(shape, float('nan'), device=self.dev) if want else None
        o5, J, g0, gt = mk(out5, (K, H, 5, n)), mk(cost, (K, n)), mk(g_obs0, (K, n, nd)), mk(g_tapes, (K, H, n, 2))
        self.api.rollout_tape_cand_vjp(self.h, n, K, H, self._ptr(obs0), self._ptr(tapes), self._ptr(ri), int(ref_ld),
                                       _path_ids(path_ids), int(path_id), int(bool(retrack)), _floats(w5),
                                       self._ptr(o5), self._ptr(J), self._ptr(g0), self._ptr(gt), self.stream)
        return o5, J, g0, gt

    # ---- include/envbuild_sample.h ----
    def sample_max(self, horizon=25):
        return self._limits('rollout_tape_sample_max', int(horizon))[0]

    def _outputs(self, want, shapes, out=None):
        """NaN-filled float tensors (best_index: int32 filled with -7) for the names in `want` that `out` does not hold yet"""
        torch = self.torch
        out = {} if out is None else out
        for k in want:
            if k not in out:
                out[k] = (torch.full(shapes[k], -7, dtype=torch.int32, device=self.dev) if k == 'best_index'
                          else torch.full(shapes[k], float('nan'), device=self.dev))
        return out

    def t_sample(self, obs0, nominal, S, ri=None, path_id=1, env_ids=None, seed=0, counter=0, sigma=(0.3, 0.3), beta=0.0, inv_lambda=1.0,
                 w5=WEIGHTS[0], want=('cost', 'best_tape', 'best_cost', 'best_index', 'mean_tape', 'samples')):
        H, n = nominal.shape[0], obs0.shape[0]
        out = self._outputs(want, dict(cost=(S, n), best_tape=(H, n, 2), best_cost=(n,), best_index=(n,), mean_tape=(H, n, 2),
                                       samples=(S, H, n, 2)))
        self.api.rollout_tape_sample(self.h, n, int(S), H, self._ptr(obs0), self._ptr(nominal), self._ptr(ri), int(path_id),
                                     self._ptr(env_ids), int(seed), int(counter), _floats(sigma), float(beta), float(inv_lambda), _floats(w5),
                                     self._ptr(out.get('cost')), self._ptr(out.get('best_tape')), self._ptr(out.get('best_cost')),
                                     self._ptr(out.get('best_index')), self._ptr(out.get('mean_tape')), self._ptr(out.get('samples')),
                                     self.stream)
        return out

    # ---- include/envbuild_ilqr.h ----
    def ilqr_max(self, horizon=25):
        return self._limits('rollout_tape_ilqr_max', int(horizon), n=2)

    def t_ilqr(self, obs0, u_nom, ri=None, path_id=1, x_nom=None, gains=None, alphas=(), mu=None, w5=WEIGHTS[0], want=ILQR_OUT, n_alpha=None,
               out=None):
        H, n = u_nom.shape[0], obs0.shape[0]
        K1 = 1 + (len(alphas) if n_alpha is None else n_alpha)
        out = self._outputs(want, dict(cost=(K1, n), best_index=(n,), best_cost=(n,), u=(H, n, 2), x=(H, 6, n), gains=(H, 14, n), dv=(2, n),
                                       cand=(K1, H, n, 2), lq=(H, 157, n)), out)
        al = None if alphas is None else (C.c_float * max(1, len(alphas)))(*[float(v) for v in alphas])
        self.api.rollout_tape_ilqr(self.h, n, H, K1 - 1, self._ptr(obs0), self._ptr(u_nom), self._ptr(x_nom), self._ptr(gains), self._ptr(ri),
                                   int(path_id), al, self._ptr(mu), _floats(w5), *[self._ptr(out.get(k)) for k in ILQR_OUT], self.stream)
        return out

    def chain_states(self, obs0, tapes, ri, pid):
        """the pre-step obs [K, H, n, D] of every step of the tapes [K, H, n, 2]: H eb_rollout_step launches over K * n rows"""
        torch = self.torch
        K, H, n = tapes.shape[0], tapes.shape[1], obs0.shape[0]
        rows = obs0.repeat(K, 1).contiguous()
        rr = None if ri is None else ri.repeat(K).contiguous()
        steps = torch.empty((H + 1, K * n, self.D), device=obs0.device)
        steps[0] = rows
        o5, sc = torch.empty((5, K * n), device=obs0.device), torch.empty((K * n, 2), device=obs0.device)
        for t in range(H):
            a = tapes[:, t].reshape(K * n, 2).contiguous()
            self.api.rollout_step(self.h, K * n, self._ptr(steps[t]), self._ptr(a), self._ptr(rr), int(pid), self._ptr(steps[t + 1]),
                                  self._ptr(o5), self._ptr(sc), self.stream)
        return steps[:H].view(H, K, n, self.D).permute(1, 0, 2, 3).contiguous()

    def unit_vjps(self, pre, tape, ri, pid, w5):
        """eb_rollout_step_vjp over the rows pre [H, n, D] with the ten cotangents of the header in ONE launch -> [H, n, 10, 11]: row
        r < 9: (g_obs_in[0..8], g_actions) for g_obs_out = e_r, g_out5 = 0; row 9: for g_obs_out = 0, g_out5 = w5"""
        torch = self.torch
        H, n, D = pre.shape
        nd = D - 4 * self.n_veh
        N = H * n * 10
        obs = pre.reshape(H * n, 1, D).expand(H * n, 10, D).reshape(N, D).contiguous()
        act = tape.reshape(H * n, 1, 2).expand(H * n, 10, 2).reshape(N, 2).contiguous()
        rr = None if ri is None else ri.view(1, n, 1).expand(H, n, 10).reshape(N).contiguous()
        g_obs = torch.zeros((H * n, 10, nd), device=pre.device)
        for r in range(9):
            g_obs[:, r, r] = 1.0
        g5 = torch.zeros((5, H * n, 10), device=pre.device)
        g5[:, :, 9] = torch.tensor([float(v) for v in w5], device=pre.device).view(5, 1)
        gi, ga = self.t_step_vjp(obs, act, rr, pid, g_obs.reshape(N, nd).contiguous(), g5.reshape(5, N).contiguous())
        return torch.cat([gi[:, :9], ga], 1).view(H, n, 10, 11)


# no family's model overrides a method of another's: one class, and the names the families' tests construct it by
CandModel = CandGradModel = SampleModel = IlqrModel = TapeModel


# ---- bit comparisons ----
def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_same(got, want, what):
    for name, a, b in zip(('out5_steps', 'obs_out', 'g_obs0', 'g_action_tape'), got, want):
        assert same(a, b), '%s: %s differs in %d of %d words' % (what, name, int((bits(a) != bits(b)).sum()), a.numel())


# ---- scenes and tapes ----
def _case_on_the_device(m, inp, ego, veh, B, H, seed):
    """what synthetic_case and edge_synthetic_case share: out-of-range ref_idx, the tracking columns, actions beyond the clip, cotangents"""
    import torch
    training = m.mode == 'training'
    ri = inp['ref_idx'].copy()
    if training:
        ri[::37] = 5                                   # out of range: no path (DAM:342, 352)
    trk = m.tracking_error(ego[:, 3], ego[:, 4], ego[:, 5], ego[:, 0], m.n_future, ref_idx=np.clip(ri, 0, 2) if training else None, path_id=1)
    obs0 = assemble_obs(ego, trk, veh)
    tape = inp['actions'].astype(np.float32)
    tape[:, ::11] *= 1.3
    g = torch.Generator(device='cuda').manual_seed(seed)
    nd = m.D - 4 * m.n_veh
    g_final = torch.randn((B, nd), device='cuda', generator=g)
    g5 = torch.randn((H, 5, B), device='cuda', generator=g)
    return m.to_dev(obs0), m.to_dev(tape), (m.to_dev(ri, np.int32) if training else None), 1, g_final, g5


def synthetic_case(m, task, B, H, seed):
    """-> obs0 [B, D], tape [H, B, 2] (a few actions beyond the +-1.05 clip), ref_idx or None, path_id, cotangents — on the device"""
    inp = make_rollout_inputs(task, B, m.n_veh, H, seed=seed, n_future=m.n_future)
    return _case_on_the_device(m, inp, inp['ego'], inp['veh'], B, H, seed)


def edge_synthetic_case(m, task, B, H, seed):
    """synthetic_case with every vehicle within 4.5 m of its ego (each record in the near queue: the queue of a tile is full), a
    third of the egos up to 400 m away (off the closest-point cell grid), a third shifted sideways onto the lane's walls"""
    inp = make_rollout_inputs(task, B, m.n_veh, H, seed=seed, n_future=m.n_future)
    rng = np.random.default_rng(seed + 1)
    ego, kind = inp['ego'], np.arange(B) % 3
    far, wall = kind == 1, kind == 2
    ego[far, 3:5] += rng.choice([-1.0, 1.0], (int(far.sum()), 2)) * rng.uniform(60.0, 380.0, (int(far.sum()), 2))
    ego[wall, 3:5] += rng.choice([-1.0, 1.0], (int(wall.sum()), 2)) * rng.uniform(0.8, 1.8, (int(wall.sum()), 2))
    rad, ang = 0.3 + 4.2 * np.sqrt(rng.random((B, m.n_veh))), rng.uniform(-np.pi, np.pi, (B, m.n_veh))
    veh = inp['veh'].reshape(B, m.n_veh, 4)
    veh[:, :, 0], veh[:, :, 1] = ego[:, 3:4] + rad * np.cos(ang), ego[:, 4:5] + rad * np.sin(ang)
    assert (np.hypot(veh[:, :, 0] - ego[:, 3:4], veh[:, :, 1] - ego[:, 4:5]) < NEAR_R - 1.0).all() and np.abs(ego[:, 3:5]).max() > 300.0
    return _case_on_the_device(m, inp, ego, veh.reshape(B, -1), B, H, seed)


def candidate_tapes(m, tape, K, seed):
    """K tapes next to `tape` [H, B, 2]: candidate 0 is the tape itself, the others seeded perturbations (some beyond the +-1.05 clip)"""
    torch = m.torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    out = [tape]
    for k in range(1, K):
        out.append(tape * (1.0 - 0.2 * k) + 0.4 * torch.randn(tape.shape, device='cuda', generator=g))
    return torch.stack(out).contiguous()


def retracked_rows(model, obs0, nf, ref_idx=None):
    """obs0 with its tracking columns replaced through ReferencePath.tracking_error_vector_batched (eb_tracking_error) for ref_idx
    [B] (training) or the model's current path (selecting)"""
    from env_build_amd.dynamics_and_models import _unwrap
    trk = model.ref_path.tracking_error_vector_batched(obs0[:, 3].contiguous(), obs0[:, 4].contiguous(), obs0[:, 5].contiguous(),
                                                       obs0[:, 0].contiguous(), nf, ref_indexes=ref_idx)
    rows = obs0.clone()
    rows[:, 6:9 + 3 * nf] = _unwrap(trk)
    return rows


def cost_in_the_headers_order(out5, w5):
    """include/envbuild_cand.h: cost = sum over ascending t from +0 of s_t; s_t = the rows with w != 0 in row order; float32, one
    rounding per operation"""
    o, w = out5.cpu().numpy(), np.asarray(w5, np.float32)
    K, H, _, B = o.shape
    J = np.zeros((K, B), np.float32)
    rows = [r for r in range(5) if w[r] != 0]
    for t in range(H if rows else 0):
        s = None
        for r in rows:
            term = o[:, t, r] * w[r]
            s = term if s is None else s + term
        J = J + s
    assert J.dtype == np.float32
    return J


# ---- the solvers' start states, the examples ----
def mpc_setup(task):
    """the G17 start rows -> (fixture, EnvironmentModel, OpenLoopMPC at the fixture's horizon, obs0, ref_idx) on the device"""
    import torch
    from env_build_amd.dynamics_and_models import EnvironmentModel
    from env_build_amd.mpc import OpenLoopMPC
    z = golden('g17_mpc_%s' % task)
    g5 = golden('g5_rollout_%s_N%d_training_nf0' % (task, NATIVE[task]))
    rows = z['rows']
    model = EnvironmentModel(task, 0, mode='training')
    obs0 = torch.from_numpy(np.ascontiguousarray(g5['obs0'][rows])).to(model.device)
    ref = torch.from_numpy(np.ascontiguousarray(g5['ref_idx'][rows].astype(np.int32))).to(model.device)
    return z, model, OpenLoopMPC(model, horizon=int(z['horizon'])), obs0, ref


def load_example(name):
    """examples/<name>.py as a module"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'examples', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the iLQR bound, on the host and on the GPU ----
def same_numbers(a, b):
    """equal as numbers (+0 and -0 alike), NaN where the other has NaN; NumPy arrays or CPU tensors"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def bound_check(got, ref32, ref64, keep, what):
    """got / ref32 / ref64: [..., C], keep: [...] bool — |got - ref64| <= 4 E + 2^-20 max|ref64| per column over the kept entries, E the
    float32 restatement's distance from the float64 one; nothing to hold when nothing is kept"""
    got, ref32, ref64 = (np.asarray(v, np.float64).reshape(-1, np.shape(v)[-1])[keep.reshape(-1)] for v in (got, ref32, ref64))
    if not len(got):
        return
    E = np.abs(ref32 - ref64).max(0)
    tol = 4.0 * E + 2.0 ** -20 * np.abs(ref64).max(0)
    err = np.abs(got - ref64).max(0)
    print('%-60s worst err / tolerance %.3f (column %d), worst err / E %.2f' % (
        what, float((err / np.maximum(tol, 1e-300)).max()), int((err / np.maximum(tol, 1e-300)).argmax()),
        float(np.where(E > 0, err / np.maximum(E, 1e-300), 0.0).max())))
    assert np.isfinite(got).all(), '%s: not finite' % what
    assert (err <= tol).all(), '%s: columns %s exceed 4 E + 2^-20 max|v64|: err %s, tol %s' % (
        what, np.nonzero(err > tol)[0], err[err > tol], tol[err > tol])


def diverged(sets_a, sets_b):
    """[H, B] bool: step t of row b, or a LATER step of it, has different active sets in a and b (the sweep runs backwards)"""
    d = sets_a != sets_b
    return np.flip(np.logical_or.accumulate(np.flip(d, 0), 0), 0)
