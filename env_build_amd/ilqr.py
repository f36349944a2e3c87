"""One iLQR / Gauss-Newton DDP iteration on the model rollout in ONE launch: rollout_tape_ilqr.

The open-loop problem of mpc.py has six ego numbers of state and two of control, closed-form dynamics, vehicles that do not depend
on the ego, and a cost that is a non-negatively weighted sum of squares.  eb_rollout_tape_ilqr (include/envbuild_ilqr.h,
csrc/eb_rollout_tape_ilqr.hip) does one iteration of the second-order method per launch: the previous feedback gains are tried at
several step lengths (closed-loop rollouts from the shared scene), the best trajectory is kept, the rollout is linearised along it
and a Riccati sweep with an exact two-dimensional box QP per step gives the next gains.

    out = rollout_tape_ilqr(model, obses, u_nom, ref_indexes=ref)                          # launch 0: no gains, candidate 0 only
    out = rollout_tape_ilqr(model, obses, out['u'], out['x'], out['gains'], alphas=(1, .5, .25), mu=mu, ref_indexes=ref)
    out['cost'] [1 + n_alpha, B], out['best_index'] [B], out['best_cost'] [B], out['u'] [H, B, 2], out['x'] [H, 6, B],
    out['gains'] [H, 14, B], out['dv'] [2, B]

feedback_actions_reference / lq_reference / riccati_reference restate the header's contract in NumPy: they are the definition a reader
checks the header against, and what the tests compare the kernel with.  lq_reference and riccati_reference run in any float dtype
(the tests run them in float32 and in float64).  fp32 state only; no CPU path: without the HIP library's entry rollout_tape_ilqr
raises.
"""
import ctypes as C

import numpy as np
import torch

from ._tape_args import check_rows, five_weights, need_fp32, path_args
from .dynamics_and_models import _dev, _stream
from .mpc import DEFAULT_WEIGHTS

__all__ = ['rollout_tape_ilqr', 'tape_ilqr_max', 'feedback_actions_reference', 'lq_reference', 'riccati_reference', 'unpack_lq',
           'GAIN_ROWS', 'LQ_ROWS', 'ACTIVE_SETS']

GAIN_ROWS, LQ_ROWS = 14, 157
# the order in which the box QP tries its active sets: (state of u_0, state of u_1), F free, L lower bound, U upper bound
ACTIVE_SETS = ('FF', 'LF', 'UF', 'FL', 'FU', 'LL', 'LU', 'UL', 'UU')
LWS = 1.4                        # (L - W) / 2: the ego's and the vehicles' circle centres (DAM:211-224)
_TRIU9 = np.triu_indices(9)


def _clamp(x):
    """x < -1 ? -1 : x > 1 ? 1 : x — a NaN stays a NaN"""
    return np.where(x < -1, x.dtype.type(-1), np.where(x > 1, x.dtype.type(1), x))


def feedback_actions_reference(u_nom, x, x_nom, gains, alpha):
    """The tape of a closed-loop candidate, bit for bit (include/envbuild_ilqr.h: candidates), in NumPy float32.
    u_nom [H, B, 2]; x [H, 6, B]: the candidate's OWN pre-step obs columns 0..5; x_nom [H, 6, B]; gains [H, 14, B]; alpha: the
    candidate's step length, or None for candidate 0 (the clamped nominal) -> u [H, B, 2]."""
    f = np.float32
    u_nom = np.asarray(u_nom, f)
    if alpha is None:
        return _clamp(u_nom)
    x, x_nom, gains = np.asarray(x, f), np.asarray(x_nom, f), np.asarray(gains, f)
    out = np.empty_like(u_nom)
    for a in range(2):
        du = f(alpha) * gains[:, a]
        for c in range(6):
            du = du + gains[:, 2 + 6 * a + c] * (x[:, c] - x_nom[:, c])
        out[:, :, a] = _clamp(u_nom[:, :, a] + du)
    return out


def _walls(task, px, py):
    """the walls of one ego point (DAM:231-295) -> [(active, weight kind, axis)]: kind 'w' = training + real, 't' / 'r' one of them"""
    if task == 'left':
        return [((py < -25) & (px < 1), 'w', 0), ((py < -25) & (3.75 - px < 1), 'w', 0), ((px < 0) & (11.25 - py < 1), 't', 1),
                ((px < -25) & (11.25 - py < 1), 'r', 1), ((px < -25) & (py - 0.0 < 1), 'w', 1)]
    if task == 'straight':
        return [((py < -25) & (px - 3.75 < 1), 'w', 0), ((py < -25) & (7.5 - px < 1), 'w', 0), ((py > 25) & (11.25 - px < 1), 'w', 0),
                ((py > 25) & (px - 0.0 < 1), 'w', 0)]
    return [((py < -25) & (px - 7.5 < 1), 'w', 0), ((py < -25) & (11.25 - px < 1), 'w', 0), ((px > 25) & (0.0 - py < 1), 'w', 1),
            ((px > 25) & (py + 11.25 < 1), 'w', 1)]


def lq_reference(task, obs, actions, weights, nd, dtype=np.float64):
    """The Gauss-Newton Hessian of one step's cost <w5, out5>, 2 sum_i c_i grad(r_i) grad(r_i)^T over the residuals active at `obs`
    (include/envbuild_ilqr.h: quadratic model), in `dtype`.  obs [B, D]: PRE-step rows; actions [B, 2] raw; nd: the first vehicle
    column -> (l_zz [B, 9, 9], l_uu [B, 2]).  The branch decisions are taken in `dtype`."""
    T = np.dtype(dtype).type
    o, a = np.asarray(obs, dtype), np.asarray(actions, dtype)
    w = [T(v) for v in weights]
    B = o.shape[0]
    d2r = T(np.pi) / T(180.0)
    lzz, luu = np.zeros((B, 9, 9), dtype), np.zeros((B, 2), dtype)
    cR = -w[0]
    # rewards (DAM:198-207, 297-298)
    lzz[:, 2, 2] = T(2 * 0.02) * cR
    lzz[:, 6, 6] = T(2 * 0.8) * cR
    lzz[:, 7, 7] = T(2 * 30.0) * d2r * d2r * cR
    lzz[:, 8, 8] = T(2 * 0.05) * cR
    passes = (a >= T(-1.05)) & (a <= T(1.05))                                   # DAM:129
    luu[:, 0] = np.where(passes[:, 0], T(2 * 5.0 * 0.4 * 0.4) * cR, T(0))
    luu[:, 1] = np.where(passes[:, 1], T(2 * 0.05 * 2.25 * 2.25) * cR, T(0))
    x, y, phi = o[:, 3], o[:, 4], o[:, 5] * d2r
    sn, cs = np.sin(phi), np.cos(phi)
    L = T(LWS)
    H3 = np.zeros((B, 3, 3), dtype)                                             # x, y, heading in radians

    def add(c, g):                                                              # H3 += 2 c g g^T per row
        H3[:] += (T(2) * c)[:, None, None] * g[:, :, None] * g[:, None, :]
    one, zero = np.ones(B, dtype), np.zeros(B, dtype)
    kinds = {'w': w[1] + w[2] + w[4], 't': w[1], 'r': w[2] + w[4]}
    for sgn in (T(1), T(-1)):
        px, py = x + sgn * L * cs, y + sgn * L * sn
        gx, gy = np.stack([one, zero, -sgn * L * sn], 1), np.stack([zero, one, sgn * L * cs], 1)
        for active, kind, axis in _walls(task, px, py):
            add(np.where(active, kinds[kind], T(0)), gx if axis == 0 else gy)
    # vehicles (DAM:218-229): the four circle pairs of every record
    veh = o[:, nd:].reshape(B, -1, 4)
    vphi = veh[:, :, 3] * d2r
    vs, vc = np.sin(vphi), np.cos(vphi)
    w35, w25 = w[1], w[2] + w[3]
    for sp in (T(1), T(-1)):
        ex, ey = (x + sp * L * cs)[:, None], (y + sp * L * sn)[:, None]
        for sq in (T(1), T(-1)):
            dx, dy = ex - (veh[:, :, 0] + sq * L * vc), ey - (veh[:, :, 1] + sq * L * vs)
            d = np.sqrt(dx * dx + dy * dy)
            c = np.where(d - T(3.5) < 0, w35, T(0)) + np.where(d - T(2.5) < 0, w25, T(0))
            ok = d > 0                                                          # a zero distance contributes zero
            dd = np.where(ok, d, T(1))
            nx, ny = dx / dd, dy / dd
            g = np.stack([nx, ny, sp * L * (ny * cs[:, None] - nx * sn[:, None])], 2)      # [B, V, 3]
            cc = np.where(ok, T(2) * c, T(0))
            H3 += (cc[:, :, None, None] * g[:, :, :, None] * g[:, :, None, :]).sum(1)
    scale = np.array([1, 1, d2r], dtype)
    lzz[:, 3:6, 3:6] = H3 * scale[None, :, None] * scale[None, None, :]        # obs column 5 is in degrees
    return lzz, luu


def unpack_lq(lq):
    """lq_out [H, 157, B] (NumPy) -> dict of A [H, B, 9, 9], B [H, B, 9, 2], l_z [H, B, 9], l_u [H, B, 2], l_zz [H, B, 9, 9], l_uu [H, B, 2]"""
    lq = np.moveaxis(np.asarray(lq), 1, 2)                                     # [H, B, 157]
    H, B = lq.shape[:2]
    lzz = np.zeros((H, B, 9, 9), lq.dtype)
    lzz[:, :, _TRIU9[0], _TRIU9[1]] = lq[:, :, 110:155]
    lzz[:, :, _TRIU9[1], _TRIU9[0]] = lq[:, :, 110:155]
    return dict(A=lq[:, :, :81].reshape(H, B, 9, 9), B=lq[:, :, 81:99].reshape(H, B, 9, 2), l_z=lq[:, :, 99:108], l_u=lq[:, :, 108:110],
                l_zz=lzz, l_uu=lq[:, :, 155:157])


def _box_qp(Q, q, lo, hi):
    """the header's box QP for a batch: Q [B, 2, 2] (= Qt_uu), q, lo, hi [B, 2] -> (d [B, 2], free [B, 2] bool, set [B], -1 = none)"""
    B = q.shape[0]
    T = q.dtype.type
    d_out, free_out, set_out = np.zeros((B, 2), q.dtype), np.zeros((B, 2), bool), np.full(B, -1)
    q00, q01, q11 = Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 1]
    with np.errstate(all='ignore'):
        for s, name in enumerate(ACTIVE_SETS):
            d = np.stack([lo[:, a] if name[a] == 'L' else hi[:, a] for a in range(2)], 1).copy()
            ok = np.ones(B, bool)
            if name == 'FF':
                det = q00 * q11 - q01 * q01
                ok = (q00 > 0) & (det > 0) & np.isfinite(q00) & np.isfinite(det)
                d[:, 0] = (q01 * q[:, 1] - q11 * q[:, 0]) / det
                d[:, 1] = (q01 * q[:, 0] - q00 * q[:, 1]) / det
            elif name[0] == 'F':
                ok = (q00 > 0) & np.isfinite(q00)
                d[:, 0] = -(q[:, 0] + q01 * d[:, 1]) / q00
            elif name[1] == 'F':
                ok = (q11 > 0) & np.isfinite(q11)
                d[:, 1] = -(q[:, 1] + q01 * d[:, 0]) / q11
            r = np.stack([(q00 * d[:, 0] + q01 * d[:, 1]) + q[:, 0], (q01 * d[:, 0] + q11 * d[:, 1]) + q[:, 1]], 1)
            for a in range(2):
                if name[a] == 'F':
                    ok = ok & (d[:, a] >= lo[:, a]) & (d[:, a] <= hi[:, a])
                elif name[a] == 'L':
                    ok = ok & (r[:, a] >= 0)
                else:
                    ok = ok & (r[:, a] <= 0)
            ok = ok & np.isfinite(d).all(1)
            take = ok & (set_out < 0)
            d_out[take] = d[take]
            free_out[take] = [name[0] == 'F', name[1] == 'F']
            set_out[take] = s
    return d_out.astype(q.dtype), free_out, set_out


def riccati_reference(A, Bm, l_z, l_u, l_zz, l_uu, u, mu=None, dtype=np.float64):
    """The backward sweep of include/envbuild_ilqr.h on a given quadratic model, in `dtype`, nine-dimensional and dense.
    A [H, B, 9, 9], Bm [H, B, 9, 2], l_z [H, B, 9], l_u [H, B, 2], l_zz [H, B, 9, 9], l_uu [H, B, 2] (diagonal), u [H, B, 2] (the
    tape the model was taken along: the box is -1 <= u + d <= 1), mu [B] or None -> (gains [H, 14, B], dv [2, B], sets [H, B])."""
    T = np.dtype(dtype).type
    A, Bm, l_z, l_u, l_zz, l_uu, u = (np.asarray(v, dtype) for v in (A, Bm, l_z, l_u, l_zz, l_uu, u))
    H, B = u.shape[:2]
    mu = np.zeros(B, dtype) if mu is None else np.asarray(mu, dtype)
    Vz, Vzz = np.zeros((B, 9), dtype), np.zeros((B, 9, 9), dtype)
    gains, dv, sets = np.zeros((H, GAIN_ROWS, B), dtype), np.zeros((2, B), dtype), np.zeros((H, B), np.int64)
    eye = np.eye(2, dtype=dtype)[None]
    At, Bt = np.swapaxes(A, -1, -2), np.swapaxes(Bm, -1, -2)
    with np.errstate(all='ignore'):
        for t in range(H - 1, -1, -1):
            Qz = l_z[t] + np.einsum('bij,bj->bi', At[t], Vz)
            Qu = l_u[t] + np.einsum('bij,bj->bi', Bt[t], Vz)
            VA = Vzz @ A[t]
            Qzz = l_zz[t] + At[t] @ VA
            Quz = Bt[t] @ VA
            Quu = Bt[t] @ (Vzz @ Bm[t])
            Quu[:, 0, 0] += l_uu[t, :, 0]
            Quu[:, 1, 1] += l_uu[t, :, 1]
            Qt = Quu + mu[:, None, None] * eye
            k, free, s = _box_qp(Qt, Qu, T(-1) - u[t], T(1) - u[t])
            K = np.zeros((B, 2, 9), dtype)
            both, only0, only1 = free[:, 0] & free[:, 1], free[:, 0] & ~free[:, 1], ~free[:, 0] & free[:, 1]
            det = Qt[:, 0, 0] * Qt[:, 1, 1] - Qt[:, 0, 1] * Qt[:, 0, 1]
            z0, z1 = Quz[:, 0], Quz[:, 1]
            K[both, 0] = ((Qt[:, 0, 1, None] * z1 - Qt[:, 1, 1, None] * z0) / det[:, None])[both]
            K[both, 1] = ((Qt[:, 0, 1, None] * z0 - Qt[:, 0, 0, None] * z1) / det[:, None])[both]
            K[only0, 0] = (-z0 / Qt[:, 0, 0, None])[only0]
            K[only1, 1] = (-z1 / Qt[:, 1, 1, None])[only1]
            Kt = np.swapaxes(K, -1, -2)
            Quuk = np.einsum('bij,bj->bi', Quu, k)
            dv[0] += (k * Qu).sum(1)
            dv[1] += (k * Quuk).sum(1)
            Vz = Qz + np.einsum('bij,bj->bi', Kt, Quuk + Qu) + np.einsum('bji,bj->bi', Quz, k)
            Vzz = Qzz + Kt @ (Quu @ K) + Kt @ Quz + np.swapaxes(Quz, -1, -2) @ K
            Vzz = T(0.5) * (Vzz + np.swapaxes(Vzz, -1, -2))
            gains[t, 0:2] = k.T
            gains[t, 2:8] = K[:, 0, :6].T
            gains[t, 8:14] = K[:, 1, :6].T
            sets[t] = s
    return gains, dv, sets


def tape_ilqr_max(model, horizon=25):
    """(the most step lengths, the longest horizon) one eb_rollout_tape_ilqr launch takes for `model`"""
    a, h = C.c_int32(0), C.c_int32(0)
    model.api.check(model.api.ilqr_fn('eb_rollout_tape_ilqr_max')(model.handle, int(horizon), C.byref(a), C.byref(h)))
    return a.value, h.value


OUTPUTS = ('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv', 'cand', 'lq')


def alloc_outputs(H, B, n_alpha, want, device):
    """the output tensors of one launch -> dict"""
    K1 = 1 + int(n_alpha)
    shapes = dict(cost=(K1, B), best_index=(B,), best_cost=(B,), u=(H, B, 2), x=(H, 6, B), gains=(H, GAIN_ROWS, B), dv=(2, B),
                  cand=(K1, H, B, 2), lq=(H, LQ_ROWS, B))
    return {k: torch.empty(shapes[k], dtype=torch.int32 if k == 'best_index' else torch.float32, device=device) for k in want}


def launch(model, obs, u_nom, x_nom, gains, alphas, mu, ref_idx, path_id, weights, out):
    """The launch behind rollout_tape_ilqr on prepared device tensors (obs [B, D], u_nom [H, B, 2], x_nom [H, 6, B] / gains [H, 14, B] or
    None, mu [B] or None: fp32 contiguous; ref_idx int32 [B] or None; alphas: a ctypes float array or a sequence) into the tensors of
    `out` (alloc_outputs; a missing key is a NULL output) -> out.  Nothing here synchronises with the host."""
    H, B = u_nom.shape[0], obs.shape[0]
    n_alpha = len(alphas)
    al = alphas if isinstance(alphas, C.Array) else (C.c_float * max(1, n_alpha))(*[float(v) for v in alphas])
    w5 = weights if isinstance(weights, C.Array) else (None if weights is None else (C.c_float * 5)(*[float(v) for v in weights]))

    def ptr(name):
        return out[name].data_ptr() if name in out and out[name].numel() else None
    rc = model.api.ilqr_fn('eb_rollout_tape_ilqr')(
        model.handle, B, H, n_alpha, obs.data_ptr(), u_nom.data_ptr(), None if x_nom is None else x_nom.data_ptr(),
        None if gains is None else gains.data_ptr(), None if ref_idx is None else ref_idx.data_ptr(), int(path_id),
        al if n_alpha else None, None if mu is None else mu.data_ptr(), w5,
        ptr('cost'), ptr('best_index'), ptr('best_cost'), ptr('u'), ptr('x'), ptr('gains'), ptr('dv'), ptr('cand'), ptr('lq'),
        _stream(model.device))
    if rc != 0:
        model.api.check(rc)
    return out


def rollout_tape_ilqr(model, obses, u_nom, x_nom=None, gains=None, alphas=(), mu=None, ref_indexes=None, path_index=None,
                      weights=DEFAULT_WEIGHTS, want=('cost', 'best_index', 'best_cost', 'u', 'x', 'gains', 'dv')):
    """One eb_rollout_tape_ilqr launch from the shared rows `obses` [B, D] along `u_nom` [H, B, 2] (raw actions) -> dict with the
    entries of `want`:
      cost [1 + n_alpha, B]     eb_rollout_tape_cand's cost of every candidate (0: the clamped nominal; j: closed-loop at alphas[j-1]);
      best_index, best_cost [B] the first minimum per env, a NaN never wins;
      u [H, B, 2], x [H, 6, B]  the best candidate's tape and its pre-step obs columns 0..5;
      gains [H, 14, B], dv [2, B]   the next feedback law (rows 0-1: k; row 2 + 6 a + c: K[a][c]) and the expected-decrease terms;
      cand [1 + n_alpha, H, B, 2], lq [H, 157, B]   the tapes as scored and the quadratic model (tests).
    x_nom [H, 6, B] and gains [H, 14, B] come together (a previous launch's x and gains) or not at all; without them alphas must be
    empty.  mu [B] >= 0 or None: the regularisation added to Q_uu's diagonal.  ref_indexes [B] (mode='training', None = the model's
    own) or path_index (mode='selecting', None = the model's current path).  `model`'s own state is not touched."""
    need_fp32(model, 'ilqr.rollout_tape_ilqr: fp32 state only')
    model.api.ilqr_fn('eb_rollout_tape_ilqr')              # EbError before any work when the library has no such entry
    want = tuple(want)
    for k in want:
        if k not in OUTPUTS:
            raise ValueError('want: a subset of %r; got %r' % (OUTPUTS, k))
    five_weights(weights, optional=True)
    obs = check_rows(model, _dev(obses, model.device).detach().contiguous())
    B = obs.shape[0]
    u = _dev(u_nom, model.device).detach().contiguous()
    if u.dim() != 3 or u.shape[1] != B or u.shape[2] != 2 or u.shape[0] < 1:
        raise ValueError('u_nom must be [H, %d, 2]; got %s' % (B, tuple(u.shape)))
    H = u.shape[0]
    xn = gn = None
    if x_nom is not None:
        xn = _dev(x_nom, model.device).detach().contiguous()
        if tuple(xn.shape) != (H, 6, B):
            raise ValueError('x_nom must be [%d, 6, %d]; got %s' % (H, B, tuple(xn.shape)))
    if gains is not None:
        gn = _dev(gains, model.device).detach().contiguous()
        if tuple(gn.shape) != (H, GAIN_ROWS, B):
            raise ValueError('gains must be [%d, %d, %d]; got %s' % (H, GAIN_ROWS, B, tuple(gn.shape)))
    m = None
    if mu is not None:
        m = _dev(mu, model.device).detach().contiguous()
        if tuple(m.shape) != (B,):
            raise ValueError('mu must be [%d]; got %s' % (B, tuple(m.shape)))
    ri, pid = path_args(model, B, ref_indexes, path_index)
    alphas = tuple(float(a) for a in alphas)
    return launch(model, obs, u, xn, gn, alphas, m, ri, pid, weights, alloc_outputs(H, B, len(alphas), want, obs.device))
