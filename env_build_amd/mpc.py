"""Batched, box-constrained open-loop MPC on the model's own cost: OpenLoopMPC.

The reference's mpc/main.py:537-576 solves, for ONE ego at a time, min_u J(u) over 25 x 2 raw actions in [-1, 1] with SciPy's SLSQP
and finite differences.  Here every env of a batch is solved at once, with the analytic gradient: one evaluation of the cost and its
gradient for the whole batch is ONE launch of eb_rollout_tape_vjp (include/envbuild_grad.h, csrc/eb_rollout_tape_vjp.hip).

Cost.   J(u) = sum_t  w . out5_t(u)      out5 = (rewards, punish_term_for_training, real_punish_term, veh2veh4real, veh2road4real)
with w = (-1, lambda, 0, 0, 0) and lambda = 10 by default: the ADP loss of examples/adp_policy_gradient.py, per env and not averaged.
(mpc/main.py carries a private cost of its own; this project's model is EnvironmentModel.rollout_out, so its outputs are the cost.)

Method. Projected gradient on the box [-1, 1]^(H x 2) (mpc/main.py:549), every env with a step length of its own: a Barzilai-Borwein
proposal, Armijo backtracking on the projected step  u+ = clip(u - a g),  J(u+) <= J(u) + c1 <g, u+ - u>.  An env whose trials are
all rejected keeps its iterate (a `where`, not a host loop) and starts the next iteration from the shortened step.  A line-search
trial is a value-only launch (g_action_tape = NULL); the update is a handful of elementwise torch ops on [H, B, 2]; nothing inside
an iteration synchronises with the host, except the optional convergence read every `check_every` iterations.
Launches per iteration: ls_trials + 1.  With fused_line_search=True the trial tapes of an iteration — they depend on u, g and the
step length only, not on each other's results — are scored by ONE eb_rollout_tape_cand launch (include/envbuild_cand.h: the scene's
vehicle records advance once for all trials): 2 launches per iteration, the same bits.  Off by default.

    mpc = OpenLoopMPC(model, horizon=25)               # model: a (Differentiable)EnvironmentModel, fp32 state
    u, J, info = mpc.solve(obses, ref_indexes=ref)     # u [H, B, 2] in [-1, 1], J [B]
    u0 = mpc.warm_start(u)                             # the tape shifted by one step: next control step's u_init
    u, J, info = mpc.solve(obses, ref_indexes=ref, u_init=torch.stack([u0, torch.zeros_like(u0)]))   # K starts: the best one per env
    J_paths, best = mpc.select_path(obses)             # the model cost of every path of the task (hier_decision.py:113-121)

Multi-start.  The cost is non-convex (collision discs), so a descent ends in the basin it starts in.  solve(..., u_init=[K, H, B, 2],
starts='all') runs EVERY start through all iterations and returns, per env, the one with the lowest final cost; solve_paths does the
same with one start per path of the task, candidate p on path p (the model-cost twin of hier_decision.py:113-121 with a tape
optimised per path).  The K gradients of an iteration are ONE eb_rollout_tape_cand_vjp launch (include/envbuild_cand_grad.h) and a
line-search trial of the K starts ONE eb_rollout_tape_cand launch, both from the shared scene: ls_trials + 1 launches per iteration
whatever K is, up to the launch limits (cand.tape_cand_grad_max, cand.tape_cand_max); see OpenLoopMPC.launch_count.

    u, J, info = mpc.solve(obses, ref_indexes=ref, u_init=starts, starts='all')   # info['J_starts'] [K, B], info['start_index'] [B]
    u, J, info = mpc.solve_paths(obses)                # info['path_index'] [B], info['J_paths'] [P, B], info['u_paths'] [P, H, B, 2]

Sampling.  SamplingMPC needs no gradient: per iteration ONE eb_rollout_tape_sample launch (include/envbuild_sample.h) draws S
perturbed tapes per env around the nominal, scores them from the shared scene and returns their soft-min average, which becomes the
next nominal (MPPI); the lowest-cost tape seen so far is kept per env.  With polish=OpenLoopMPC(...) it is the global stage in front
of the gradient solver: the sampled tape and the zero tape both descend (starts='all'), so the result is never above the default
solver's.

    smpc = SamplingMPC(model, horizon=25, n_samples=256)
    u, J, info = smpc.solve(obses, ref_indexes=ref)    # info['J_history'] [iterations + 1, B], info['counter_next']

Second order.  ILQRMPC is iLQR / Gauss-Newton DDP with an exact box QP per step: per iteration ONE eb_rollout_tape_ilqr launch
(include/envbuild_ilqr.h) tries the previous feedback gains at several step lengths, keeps the best trajectory, linearises along it
and sweeps backwards to the next gains.  A solve is iterations + 2 launches and reads nothing on the host.  polish works as
SamplingMPC's.

    impc = ILQRMPC(model, horizon=25)
    u, J, info = impc.solve(obses, ref_indexes=ref)    # info['J_history'] [iterations + 1, B], info['best_index'], info['mu']
"""
import ctypes as C

import torch

from ._tape_args import check_rows, five_weights, need_fp32, tapes_or_zeros

__all__ = ['OpenLoopMPC', 'SamplingMPC', 'ILQRMPC', 'cost_from_out5', 'projected_gradient', 'sampling_loop', 'ilqr_loop', 'best_start',
           'DEFAULT_WEIGHTS']

DEFAULT_WEIGHTS = (-1.0, 10.0, 0.0, 0.0, 0.0)


def cost_from_out5(out5_steps, weights=DEFAULT_WEIGHTS):
    """J [B] = sum_t w . out5_steps[t] from out5_steps [H, 5, B], in ONE fixed order: per step the non-zero weights' terms are added
    in row order (k = 0..4), then one torch reduction over the steps (its order is fixed by the shape and the device, and an env's
    sum does not involve its neighbours).  The solver and its tests form J with this function only."""
    w = [float(v) for v in weights]
    per_step = None
    for k in range(5):
        if w[k] != 0.0:
            term = out5_steps[:, k] * w[k]
            per_step = term if per_step is None else per_step + term
    if per_step is None:
        return torch.zeros_like(out5_steps[0, 0])
    return per_step.sum(0)


def first_minimum(J):
    """index [B] of every env's lowest cost in J [K, B]: the first minimum; a NaN never wins; all NaN gives 0"""
    best = torch.where(torch.isnan(J[0]), torch.full_like(J[0], float('inf')), J[0])
    idx = torch.zeros(J.shape[1], dtype=torch.long, device=J.device)
    for k in range(1, J.shape[0]):
        better = J[k] < best                                         # strict: the first minimum; False for NaN
        idx = torch.where(better, torch.full_like(idx, k), idx)
        best = torch.where(better, J[k], best)
    return idx


def best_start(U, evaluate_many):
    """Of K starts U [K, H, B, 2] every env's lowest-cost one, scored by ONE evaluate_many call: -> (u [H, B, 2], index [B], J [K, B]).
    The first minimum wins; a NaN cost never wins; an env whose costs are all NaN gets start 0."""
    U = U.clamp(-1.0, 1.0)
    J = evaluate_many(U)
    idx = first_minimum(J)
    u = U.gather(0, idx.view(1, 1, -1, 1).expand(1, U.shape[1], U.shape[2], 2))[0]
    return u.contiguous(), idx, J


def projected_gradient(evaluate, u, iterations, ls_trials=3, c1=1e-4, shrink=0.25, alpha_min=1e-8, alpha_max=1e2, check_every=0,
                       tol=1e-3, evaluate_many=None):
    """min J(u) over the box [-1, 1] for a batch of independent problems.
        evaluate(u [H, B, 2], need_grad) -> (J [B], g [H, B, 2] or None)
    or, with a leading start dimension, K * B independent problems, each with its own step length, Armijo state and BB proposal:
        evaluate(U [K, H, B, 2], need_grad) -> (J [K, B], g [K, H, B, 2] or None)
    (J_history is then [iterations + 1, K, B], accepted [iterations, K, B]; the reduced dimensions are counted from the end, so the
    [H, B, 2] form runs the lines it always ran).
    Tensors of any float dtype and device (the GPU solver runs it in float32 on the device, the fixture generator in float64 on the
    CPU: the same lines).  -> (u, J, info); info: J_history [iterations + 1, B] (J after every iteration: accepted steps only, so it
    never increases), accepted [iterations, B], iterations (done), evaluations.
        evaluate_many(U [T, H, B, 2]) -> J [T, B]   (optional; with a start dimension U [T, K, H, B, 2] -> J [T, K, B])
    With it the ls_trials trial tapes of an iteration are formed up front — their step lengths a, a shrink, (a shrink) shrink, ... by
    repeated multiplication, as the sequential loop forms them for an env that has not accepted yet — scored by ONE call and accepted
    by the same rule in trial order.  A trial after an env's accepted one is scored and ignored (sequentially it would have been
    scored at the accepted step length and ignored), so u, J, J_history and accepted are those of the sequential loop bit for bit
    whenever evaluate_many(U)[k] == evaluate(U[k], False)[0]."""
    def env(v):                                                      # [B] -> [1, B, 1]; [K, B] -> [K, 1, B, 1]
        return v.unsqueeze(-1).unsqueeze(-3)
    u = u.clamp(-1.0, 1.0)
    J, g = evaluate(u, True)
    n_eval = 1
    # first step: no env moves an action by more than 1 (half the box)
    alpha = (1.0 / g.abs().amax((-3, -1)).clamp_min(1e-12)).clamp(alpha_min, alpha_max)
    hist, acc = [J], []
    done_iters = 0
    U = None
    for it in range(iterations):
        a = alpha
        u_new, J_new = u, J
        done = torch.zeros_like(J, dtype=torch.bool)
        J_many = None
        if evaluate_many is not None:
            if U is None:                                            # the trial tapes' buffer [T, ...]: one for the whole solve
                U = torch.empty((ls_trials,) + tuple(u.shape), dtype=u.dtype, device=u.device)
            steps = [a]
            for k in range(ls_trials):
                torch.clamp(u - env(steps[k]) * g, -1.0, 1.0, out=U[k])
                steps.append(steps[k] * shrink)
            tries = [U[k] for k in range(ls_trials)]
            J_many = evaluate_many(U)
        for k in range(ls_trials):
            if J_many is None:
                u_try = (u - env(a) * g).clamp(-1.0, 1.0)
                J_try, _g = evaluate(u_try, False)
            else:
                u_try, J_try = tries[k], J_many[k]
            n_eval += 1
            slope = ((u_try - u) * g).sum((-3, -1))                   # <= 0: the projected step is a descent direction
            ok = (J_try <= J + c1 * slope) & ~done                   # a NaN cost is a rejection
            u_new = torch.where(env(ok), u_try, u_new)
            J_new = torch.where(ok, J_try, J_new)
            done = done | ok
            a = torch.where(done, a, a * shrink if J_many is None else steps[k + 1])   # (an env not done yet: a == steps[k])
        _J, g_new = evaluate(u_new, True)                            # the same bits as J_new: value-only == the full form's forward
        n_eval += 1
        s, y = u_new - u, g_new - g
        ss, sy = (s * s).sum((-3, -1)), (s * y).sum((-3, -1))
        bb = torch.where(sy > 0, ss / sy.clamp_min(1e-30), a * 4.0)  # BB1; non-positive curvature along s: lengthen
        alpha = torch.where(done, bb, a).clamp(alpha_min, alpha_max)  # a rejected env goes on from its shortened step
        u, J, g = u_new, J_new, g_new
        hist.append(J)
        acc.append(done)
        done_iters = it + 1
        if check_every and (it + 1) % check_every == 0 and it + 1 >= check_every:
            if float((hist[-1 - check_every] - J).max()) <= tol:    # the one host read
                break
    info = dict(J_history=torch.stack(hist), accepted=torch.stack(acc) if acc else torch.zeros((0,) + J.shape, dtype=torch.bool),
                iterations=done_iters, evaluations=n_eval, launches_per_iteration=ls_trials + 1 if evaluate_many is None else 2)
    return u, J, info


def _solve_path_args(model, dev_fn, ref_indexes, path_index, who):
    """the path arguments of a solve -> (ref_idx int32 [B] on the device or None, path id)"""
    if model.mode == 'training':
        if ref_indexes is None:
            raise ValueError("%s: mode='training' needs ref_indexes [B]" % who)
        return dev_fn(ref_indexes, model.device, torch.int32), 0
    if path_index is None:
        raise ValueError("%s: mode='selecting' needs path_index" % who)
    return None, int(path_index)


class OpenLoopMPC(object):
    """Open-loop MPC over `horizon` steps of `model` (task, slot modes, mode and path tables are the model's).  fp32 state only."""

    def __init__(self, model, horizon=25, weights=DEFAULT_WEIGHTS, iterations=60, ls_trials=3, c1=1e-4, fused_line_search=False):
        from .dynamics_and_models import _dev, _stream
        self._dev_fn, self._stream_fn = _dev, _stream
        need_fp32(model, 'OpenLoopMPC: the reverse pass is fp32-state only')
        self.model, self.horizon = model, int(horizon)
        self.weights = five_weights(weights)
        self.iterations, self.ls_trials, self.c1 = int(iterations), int(ls_trials), float(c1)
        self._fn = model.api.grad_fn('eb_rollout_tape_vjp')          # EbError here when the library has no reverse pass
        limit = C.c_int32(0)
        model.api.check(model.api.grad_fn('eb_rollout_tape_vjp_max_horizon')(model.handle, C.byref(limit)))
        if self.horizon < 1 or self.horizon > limit.value:
            raise ValueError('OpenLoopMPC: horizon %d is outside 1..%d (eb_rollout_tape_vjp_max_horizon)' % (self.horizon, limit.value))
        self._w5 = (C.c_float * 5)(*self.weights)
        self.fused_line_search = bool(fused_line_search)
        if self.fused_line_search:
            model.api.cand_fn('eb_rollout_tape_cand')                # EbError here when the library has no candidate-tape rollout
        self.launches = 0

    # -- one launch ------------------------------------------------------------------------------
    def value_and_grad(self, obs, u, ref_idx, path_id, need_grad=True):
        """-> (J [B], dJ/du [H, B, 2] or None, out5_steps [H, 5, B]): one eb_rollout_tape_vjp launch on the current stream"""
        m = self.model
        H, B = u.shape[0], obs.shape[0]
        out5 = torch.empty((H, 5, B), dtype=torch.float32, device=obs.device)
        g = torch.empty_like(u) if need_grad else None
        rc = self._fn(m.handle, B, H, obs.data_ptr(), u.data_ptr(), None if ref_idx is None else ref_idx.data_ptr(), path_id,
                      None, 0, None, self._w5, out5.data_ptr(), None, None, None if g is None else g.data_ptr(),
                      self._stream_fn(m.device))
        if rc != 0:
            m.api.check(rc)
        self.launches += 1
        return cost_from_out5(out5, self.weights), g, out5

    def values_many(self, obs, U, ref_idx, path_id):
        """-> J [K, B] of K tapes U [K, H, B, 2] from the shared rows `obs`: one eb_rollout_tape_cand launch (per tape_cand_max
        candidates) with out5_steps, and cost_from_out5 per candidate slice — J is formed by the lines value_and_grad forms it with"""
        from .cand import launch_chunks
        ids = None if ref_idx is not None else [path_id] * U.shape[0]
        out5, _cost, launches = launch_chunks(self.model, obs, U.contiguous(), ref_idx, ids, False, None, True)
        self.launches += launches
        return torch.stack([cost_from_out5(out5[k], self.weights) for k in range(U.shape[0])])

    def _many(self, obs, U, ri, ids, retrack, need_grad):
        """Cost (and gradient) of N tapes U [N, H, B, 2] from the shared rows `obs`, tape i on path ri[i] ([N, B]; [B]: one path for
        all) or ids[i] -> (J [N, B], g [N, H, B, 2] or None).  need_grad: eb_rollout_tape_cand_vjp, else eb_rollout_tape_cand, in
        chunks of their limits; J is cost_from_out5 per candidate slice of out5_steps — the lines value_and_grad forms it with."""
        from .cand import launch_chunks, launch_grad_chunks
        g = None
        if need_grad:
            _cost, g, out5, _g_obs, launches = launch_grad_chunks(self.model, obs, U, ri, ids, retrack, self.weights, True, False)
        else:
            out5, _cost, launches = launch_chunks(self.model, obs, U, ri, ids, retrack, None, True)
        self.launches += launches
        return torch.stack([cost_from_out5(out5[k], self.weights) for k in range(U.shape[0])]), g

    def launch_count(self, n_starts, iterations):
        """Launches of a solve(starts='all') / solve_paths over n_starts starts that runs `iterations` iterations:
            G + iterations * (V + G),   G = ceil(K / tape_cand_grad_max),
            V = ls_trials * ceil(K / tape_cand_max)   or, with fused_line_search,   ceil(K * ls_trials / tape_cand_max)
        (one gradient evaluation in front, then per iteration the line search's value-only launches and one gradient evaluation).
        For K up to tape_cand_grad_max that is 1 + iterations * (ls_trials + 1), independent of K."""
        from .cand import tape_cand_grad_max, tape_cand_max
        K = int(n_starts)
        G = -(-K // max(1, tape_cand_grad_max(self.model, self.horizon)))
        lim = tape_cand_max(self.model, self.horizon)
        V = -(-K * self.ls_trials // lim) if self.fused_line_search else self.ls_trials * -(-K // lim)
        return G + int(iterations) * (V + G)

    def _solve_all(self, obs, U0, ri, ids, retrack, iterations, check_every, tol):
        """every start of U0 [K, H, B, 2] through projected_gradient at once -> (U [K, H, B, 2], J [K, B], info)"""
        K = U0.shape[0]
        per_cand = ri is not None and ri.dim() == 2

        def evaluate(U, need_grad):
            return self._many(obs, U.contiguous(), ri, ids, retrack, need_grad)

        def evaluate_many(UU):                                       # [T, K, H, B, 2]: trial t of start k is candidate t * K + k
            T = UU.shape[0]
            J, _g = self._many(obs, UU.reshape((T * K,) + tuple(UU.shape[2:])), ri.repeat(T, 1) if per_cand else ri,
                               None if ids is None else ids * T, retrack, False)
            return J.view(T, K, -1)
        first = self.launches
        U, J, info = projected_gradient(evaluate, U0, self.iterations if iterations is None else int(iterations),
                                        ls_trials=self.ls_trials, c1=self.c1, check_every=check_every, tol=tol,
                                        evaluate_many=evaluate_many if self.fused_line_search else None)
        info['launches'] = self.launches - first
        return U, J, info

    @staticmethod
    def _pick(U, J):
        """per env the start with the lowest cost (first_minimum) -> (u [H, B, 2], J [B], index [B])"""
        idx = first_minimum(J)
        u = U.gather(0, idx.view(1, 1, -1, 1).expand(1, U.shape[1], U.shape[2], 2))[0]
        return u.contiguous(), J.gather(0, idx.view(1, -1))[0], idx

    def _per_path(self, obses, tapes, what):
        """one candidate per path of the task -> (obs [B, D], tapes [P, H, B, 2] (None = zeros), ref_idx [P, B] or None, path ids or None)"""
        m = self.model
        obs = check_rows(m, self._dev_fn(obses, m.device).detach())
        P, B = len(m.ref_path.path_list), obs.shape[0]
        U = tapes_or_zeros(m, tapes, (P, self.horizon, B, 2), what)
        if m.mode == 'training':
            return obs, U, torch.arange(P, dtype=torch.int32, device=m.device).view(P, 1).expand(P, B).contiguous(), None
        return obs, U, None, list(range(P))

    def solve_paths(self, obses, u_init=None, iterations=None, check_every=0, tol=1e-3):
        """One start per path of the task, candidate p on path p from the row's tracking error on THAT path (retrack; the reference
        builds one obs per path, hier_decision.py:113-117), all optimised together; the best path per env is returned — "optimise a
        tape per path, then compare" (hier_decision.py:113-121 on the model cost) -> (u [H, B, 2], J [B], info).
        u_init: None = the zero tapes, or [P, H, B, 2].  info as projected_gradient's with a start dimension, plus path_index [B] (the
        first minimum; a NaN never wins), J_paths [P, B], u_paths [P, H, B, 2], launches (launch_count(P, iterations)).  The
        hysteresis of hier_decision.py:121 stays with the caller."""
        obs, U0, ri, ids = self._per_path(obses, u_init, 'u_init')
        U, J, info = self._solve_all(obs, U0, ri, ids, True, iterations, check_every, tol)
        u, J_best, idx = self._pick(U, J)
        info.update(path_index=idx, J_paths=J, u_paths=U.contiguous())
        return u, J_best, info

    def select_path(self, obses, tapes=None):
        """The model cost of every path of the task from the shared rows `obses` [B, D] — the model-cost twin of
        hier_decision.py:113-121 -> (J [P, B], best [B]: the first minimum).  Candidate p follows path p for every env and starts from
        the row's tracking error on THAT path (retrack: the reference builds one obs per path, hier_decision.py:113-117); tapes
        [P, H, B, 2] or None = the zero tapes.  J is eb_rollout_tape_cand's `cost` with this solver's weights.  One launch; the
        hysteresis of hier_decision.py:121 stays with the caller."""
        from .cand import launch_chunks
        obs, U, ri, ids = self._per_path(obses, tapes, 'tapes')
        _out5, J, launches = launch_chunks(self.model, obs, U, ri, ids, True, self.weights, False)
        self.launches += launches
        return J, first_minimum(J)

    def _paths(self, ref_indexes, path_index):
        return _solve_path_args(self.model, self._dev_fn, ref_indexes, path_index, 'OpenLoopMPC.solve')

    def solve(self, obses, ref_indexes=None, path_index=None, u_init=None, iterations=None, check_every=0, tol=1e-3, starts='best'):
        """-> (u [H, B, 2] raw actions in [-1, 1], J [B], info).  u_init: None = the zero tape (mpc/main.py:550), or a tape
        [H, B, 2] (warm_start), or K starts [K, H, B, 2].  starts='best' (the default): the K starts are scored by one
        eb_rollout_tape_cand launch and every env starts ONE descent from its lowest-cost one (best_start; info['start_index'] [B]).
        starts='all': every start runs through all iterations (one eb_rollout_tape_cand_vjp launch per gradient evaluation of the K
        starts) and every env gets the start with the lowest FINAL cost — the first minimum, a NaN never wins; info then has
        J_history [iterations + 1, K, B], accepted [iterations, K, B], J_starts [K, B], start_index [B] and launches ==
        launch_count(K, iterations).  info otherwise as projected_gradient's, plus `launches`."""
        if starts not in ('best', 'all'):
            raise ValueError("starts must be 'best' or 'all'; got %r" % (starts,))
        m = self.model
        obs = check_rows(m, self._dev_fn(obses, m.device).detach())
        B = obs.shape[0]
        ri, pid = self._paths(ref_indexes, path_index)
        if u_init is None:
            u0 = torch.zeros((self.horizon, B, 2), dtype=torch.float32, device=m.device)
        else:
            u0 = self._dev_fn(u_init, m.device).detach()
            if tuple(u0.shape[-3:]) != (self.horizon, B, 2) or u0.dim() not in (3, 4) or (u0.dim() == 4 and u0.shape[0] < 1):
                raise ValueError('u_init must be [%d, %d, 2] or [K, %d, %d, 2]; got %s' % (self.horizon, B, self.horizon, B, tuple(u0.shape)))
        if starts == 'all':
            if u0.dim() != 4:
                raise ValueError("starts='all' needs u_init [K, %d, %d, 2]" % (self.horizon, B))
            U, J_starts, info = self._solve_all(obs, u0, ri, None if ri is not None else [pid] * u0.shape[0], False, iterations,
                                                check_every, tol)
            u, J, idx = self._pick(U, J_starts)
            info.update(J_starts=J_starts, start_index=idx)
            return u, J, info
        first = self.launches
        start_index = None
        if u0.dim() == 4:
            u0, start_index, _ = best_start(u0, lambda U: self.values_many(obs, U, ri, pid))

        def evaluate(u, need_grad):
            J, g, _ = self.value_and_grad(obs, u.contiguous(), ri, pid, need_grad)
            return J, g
        u, J, info = projected_gradient(evaluate, u0, self.iterations if iterations is None else int(iterations),
                                        ls_trials=self.ls_trials, c1=self.c1, check_every=check_every, tol=tol,
                                        evaluate_many=(lambda U: self.values_many(obs, U, ri, pid)) if self.fused_line_search else None)
        info['launches'] = self.launches - first
        if start_index is not None:
            info['start_index'] = start_index
        return u.contiguous(), J, info

    @staticmethod
    def warm_start(u):
        """The tape shifted by one step, its last action repeated: the next control step's u_init (the line mpc/main.py:571 left
        commented out)."""
        return torch.cat([u[1:], u[-1:]], 0).contiguous()


def _finish(mpc, obs, u, J_kernel, info, ri, pid, first, prefix):
    """The tail of SamplingMPC.solve and ILQRMPC.solve: ONE independent value-only evaluation of the stage's tape u gives the returned
    J; with mpc.polish the zero tape and u then go through polish.solve(starts='all') and info keeps the stage's own result as
    u_<prefix> / J_<prefix>.  first: mpc.launches when the solve began.  -> (u, J, info)"""
    u = u.contiguous()
    J = mpc._value.value_and_grad(obs, u, ri, pid, need_grad=False)[0]
    mpc.launches += 1
    info.update(J_kernel=J_kernel, launches=mpc.launches - first)
    if mpc.polish is not None:
        starts = torch.stack([torch.zeros_like(u), u])
        up, Jp, pinfo = mpc.polish.solve(obs, ref_indexes=ri, path_index=None if ri is not None else pid, u_init=starts, starts='all')
        info.update({'u_' + prefix: u, 'J_' + prefix: J}, polish=pinfo, launches=info['launches'] + pinfo['launches'])
        u, J = up, Jp
    return u, J, info


def sampling_loop(step, u0, iterations, sigma, sigma_decay=1.0, counter=0):
    """The MPPI iteration on a batch of independent problems, free of the device:
        step(nominal [H, B, 2], counter, (sigma_0, sigma_1)) -> (cost0 [B], best_tape [H, B, 2], best_cost [B], mean_tape [H, B, 2])
    is one sampling step around `nominal` (cost0: the cost of the nominal itself, sample 0).  Per iteration: one step; the nominal
    becomes mean_tape; the lowest-cost tape seen so far is kept per env with a `where` (elitist; a NaN never replaces anything, so an
    env whose costs are all NaN keeps its start); the counter advances by one and sigma is multiplied by sigma_decay.  Nothing here
    reads a value on the host.  -> (u [H, B, 2], J [B], info): J_history [iterations + 1, B] (J_history[0]: the start's cost; it
    never increases), counter_next."""
    nominal = u0.clamp(-1.0, 1.0)
    u_best, J_best = nominal, None
    sig = (float(sigma[0]), float(sigma[1]))
    hist = []
    for it in range(int(iterations)):
        cost0, best_tape, best_cost, mean_tape = step(nominal, int(counter) + it, sig)
        if J_best is None:
            J_best = cost0
            hist.append(J_best)
        floor = torch.where(torch.isnan(J_best), torch.full_like(J_best, float('inf')), J_best)
        better = best_cost < floor                                   # strict; False for a NaN
        u_best = torch.where(better.view(1, -1, 1), best_tape, u_best)
        J_best = torch.where(better, best_cost, J_best)
        hist.append(J_best)
        nominal = mean_tape
        sig = (sig[0] * float(sigma_decay), sig[1] * float(sigma_decay))
    info = dict(J_history=torch.stack(hist) if hist else None, counter_next=int(counter) + int(iterations))
    return u_best, J_best, info


class SamplingMPC(object):
    """Sampling MPC (MPPI) over `horizon` steps of `model`: n_samples perturbed tapes per env and iteration, one
    eb_rollout_tape_sample launch each.  sigma: the noise scale per action component (raw actions live in [-1, 1]), multiplied by
    sigma_decay after every iteration; beta: AR(1) smoothing of the noise over the steps; lam: the soft-min temperature in units of
    the cost; seed: with solve's `counter` it keys every draw, so a solve repeats its bits.  polish: an OpenLoopMPC on the same
    model, horizon and weights, or None.  fp32 state only."""

    def __init__(self, model, horizon=25, weights=DEFAULT_WEIGHTS, n_samples=256, iterations=8, sigma=(0.4, 0.4), beta=0.7, lam=1.0,
                 sigma_decay=0.85, seed=0, polish=None):
        from .dynamics_and_models import _dev
        from . import sample as _sample
        self._dev_fn, self._sample = _dev, _sample
        need_fp32(model, 'SamplingMPC: fp32 state only')
        model.api.sample_fn('eb_rollout_tape_sample')                # EbError here when the library has no sampled-tape rollout
        self.model, self.horizon = model, int(horizon)
        self.weights = five_weights(weights)
        self.n_samples, self.iterations = int(n_samples), int(iterations)
        limit = _sample.tape_sample_max(model, self.horizon)         # ValueError for a horizon outside 1..128
        if self.n_samples < 1 or self.n_samples > limit:
            raise ValueError('SamplingMPC: n_samples %d is outside 1..%d (eb_rollout_tape_sample_max)' % (self.n_samples, limit))
        if self.iterations < 1:
            raise ValueError('SamplingMPC: at least one iteration')
        self.sigma = (float(sigma[0]), float(sigma[1]))
        self.beta, self.lam, self.sigma_decay, self.seed = float(beta), float(lam), float(sigma_decay), int(seed)
        if not self.lam > 0:
            raise ValueError('SamplingMPC: lam must be positive')
        self.polish = polish
        if polish is not None and (polish.model is not model or polish.horizon != self.horizon or polish.weights != self.weights):
            raise ValueError('SamplingMPC: polish must be an OpenLoopMPC on the same model, horizon and weights')
        self._value = OpenLoopMPC(model, horizon=self.horizon, weights=self.weights)      # the independent evaluation of the result
        self.launches = 0

    def solve(self, obses, ref_indexes=None, path_index=None, u_init=None, counter=0):
        """-> (u [H, B, 2] raw actions in [-1, 1], J [B], info).  u_init: None = the zero tape, or a tape [H, B, 2] (warm_start).
        J is cost_from_out5 of ONE independent value-only evaluation of the returned u (the contract of OpenLoopMPC.solve).
        info: J_history [iterations + 1, B] (the best cost after every iteration, as the sampling kernel formed it: it never
        increases), J_kernel [B] (= J_history[-1]; it agrees with J to the rounding of the two summation orders), launches
        (iterations + 1), counter_next (the counter a following solve continues from).  With polish the sampled tape and the zero
        tape go through polish.solve(u_init=stack([zero, u_sampled]), starts='all') — start 0 is the zero tape on purpose: its
        descent is the default solver's — and u, J are the polished ones; info then also has u_sampled, J_sampled and `polish`
        (polish.solve's info), and launches counts both stages."""
        m = self.model
        obs = check_rows(m, self._dev_fn(obses, m.device).detach())
        B = obs.shape[0]
        ri, pid = _solve_path_args(m, self._dev_fn, ref_indexes, path_index, 'SamplingMPC.solve')
        u0 = tapes_or_zeros(m, u_init, (self.horizon, B, 2), 'u_init')
        inv = 0.0 if self.lam == float('inf') else 1.0 / self.lam
        first = self.launches

        def step(nominal, cnt, sig):
            out = self._sample.launch(m, obs, nominal.contiguous(), self.n_samples, self.seed, cnt, sig, self.beta, inv, ri, pid, None,
                                      self.weights, ('cost', 'best', 'mean'))
            self.launches += 1
            return out['cost'][0], out['best_tape'], out['best_cost'], out['mean_tape']
        u, J_kernel, info = sampling_loop(step, u0, self.iterations, self.sigma, self.sigma_decay, counter)
        return _finish(self, obs, u, J_kernel, info, ri, pid, first, 'sampled')

    warm_start = staticmethod(OpenLoopMPC.warm_start)


def ilqr_loop(step, u0, iterations, mu0=0.0):
    """The iLQR iteration on a batch of independent problems, free of the device:
        step(u_nom [H, B, 2], x_nom, gains, mu [B] or None, need_gains) -> dict(best_index [B], best_cost [B], u, x, gains)
    is one iteration along u_nom: candidate 0 is u_nom itself, candidates j >= 1 follow the feedback law (x_nom, gains) at the step
    lengths of the caller; u / x / gains are the best candidate's tape, its states and the NEXT gains (None / None / None on the
    first call: candidate 0 only).  need_gains is False on the LAST call, whose gains nobody reads: the step may skip its backward
    sweep and leave `gains` out.  step may hand out the same two sets of tensors in turn (ping-pong): what is kept here is cloned.
    Per env the regularisation mu becomes max(10 mu, 1e-3), capped at 1e6, when candidate 0 won (no step length helped), else 0.2 mu,
    flushed to 0 below 1e-6 — a `where`, nothing is read on the host.
    -> (u [H, B, 2], J [B], info): J_history [iterations + 1, B] (it never increases: candidate 0 is always in the set), best_index
    [iterations, B], mu [B] (after the last iteration)."""
    n_it = int(iterations)
    out = step(u0, None, None, None, n_it > 0)
    J = out['best_cost']
    mu = torch.full_like(J, float(mu0))
    hist, picks = [J.clone()], []
    for it in range(n_it):
        out = step(out['u'], out['x'], out['gains'], mu, it + 1 < n_it)
        stay = out['best_index'] == 0
        down = 0.2 * mu
        mu = torch.where(stay, (10.0 * mu).clamp(1e-3, 1e6), torch.where(down < 1e-6, torch.zeros_like(mu), down))
        hist.append(out['best_cost'].clone())
        picks.append(out['best_index'].clone())
    info = dict(J_history=torch.stack(hist), mu=mu,
                best_index=torch.stack(picks) if picks else torch.zeros((0,) + tuple(J.shape), dtype=torch.int32, device=J.device))
    return out['u'].clone(), hist[-1], info


class ILQRMPC(object):
    """Second-order MPC (iLQR / Gauss-Newton DDP, box-constrained) over `horizon` steps of `model`: one eb_rollout_tape_ilqr launch per
    iteration.  alphas: the step lengths every iteration tries (at most ilqr.tape_ilqr_max's); mu0: the start value of the per-env
    regularisation of Q_uu; weights must satisfy w[0] <= 0 and w[1..4] >= 0 (a sum of squares).  polish: an OpenLoopMPC on the same
    model, horizon and weights, or None.  fp32 state only."""

    def __init__(self, model, horizon=25, weights=DEFAULT_WEIGHTS, iterations=15, alphas=(1, .5, .25, .125, .0625, .03125, .015625),
                 mu0=0.0, polish=None):
        from .dynamics_and_models import _dev
        from . import ilqr as _ilqr
        self._dev_fn, self._ilqr = _dev, _ilqr
        need_fp32(model, 'ILQRMPC: fp32 state only')
        model.api.ilqr_fn('eb_rollout_tape_ilqr')                    # EbError here when the library has no iLQR iteration
        self.model, self.horizon = model, int(horizon)
        self.weights = five_weights(weights)
        if self.weights[0] > 0 or min(self.weights[1:]) < 0:
            raise ValueError('ILQRMPC: weights must satisfy w[0] <= 0 and w[1..4] >= 0')
        self.iterations = int(iterations)
        if self.iterations < 0:
            raise ValueError('ILQRMPC: iterations must not be negative')
        self.alphas = tuple(float(a) for a in alphas)
        max_alpha, max_h = _ilqr.tape_ilqr_max(model, self.horizon)
        if self.horizon < 1 or self.horizon > max_h:
            raise ValueError('ILQRMPC: horizon %d is outside 1..%d (eb_rollout_tape_ilqr_max)' % (self.horizon, max_h))
        if len(self.alphas) < 1 or len(self.alphas) > max_alpha or not all(0 < a < float('inf') for a in self.alphas):
            raise ValueError('ILQRMPC: 1..%d finite positive step lengths (eb_rollout_tape_ilqr_max)' % max_alpha)
        self.mu0 = float(mu0)
        if not self.mu0 >= 0:
            raise ValueError('ILQRMPC: mu0 must not be negative')
        self.polish = polish
        if polish is not None and (polish.model is not model or polish.horizon != self.horizon or polish.weights != self.weights):
            raise ValueError('ILQRMPC: polish must be an OpenLoopMPC on the same model, horizon and weights')
        self._value = OpenLoopMPC(model, horizon=self.horizon, weights=self.weights)      # the independent evaluation of the result
        self._al = (C.c_float * len(self.alphas))(*self.alphas)
        self._w5 = (C.c_float * 5)(*self.weights)
        self._buffers = None
        self.launches = 0

    def _ping_pong(self, B, device):
        """the two sets of output tensors of a solve, allocated once per (batch size, device)"""
        key = (B, str(device))
        if self._buffers is None or self._buffers[0] != key:
            want = ('cost', 'best_index', 'best_cost', 'u', 'x', 'gains')
            first = self._ilqr.alloc_outputs(self.horizon, B, 0, want, device)
            sets = [self._ilqr.alloc_outputs(self.horizon, B, len(self.alphas), want, device) for _ in range(2)]
            self._buffers = (key, first, sets)
        return self._buffers[1], self._buffers[2]

    def solve(self, obses, ref_indexes=None, path_index=None, u_init=None):
        """-> (u [H, B, 2] raw actions in [-1, 1], J [B], info).  u_init: None = the zero tape, or a tape [H, B, 2] (warm_start).
        Launch 0 has no gains (it scores the start and linearises along it); then `iterations` launches, each consuming the previous
        one's u / x / gains through two sets of buffers allocated once (the last one asks for no gains: it is the value-only form); then ONE independent value-only eb_rollout_tape_vjp launch
        whose cost_from_out5 is the returned J (the contract of OpenLoopMPC.solve).  info: J_history [iterations + 1, B] (the best cost
        after launch 0 and after every iteration, as the kernel formed it: it never increases), best_index [iterations, B] (0: no step
        length helped), mu [B], J_kernel [B] (= J_history[-1]; it agrees with J to the rounding of the two summation orders),
        launches (iterations + 2).  With polish the zero tape and the iLQR tape go through
        polish.solve(u_init=stack([zero, u_ilqr]), starts='all') — start 0 is the zero tape on purpose: its descent is the default
        solver's — and u, J are the polished ones; info then also has u_ilqr, J_ilqr and `polish`, and launches counts both stages."""
        m = self.model
        obs = check_rows(m, self._dev_fn(obses, m.device).detach().contiguous())
        B = obs.shape[0]
        ri, pid = _solve_path_args(m, self._dev_fn, ref_indexes, path_index, 'ILQRMPC.solve')
        u0 = tapes_or_zeros(m, u_init, (self.horizon, B, 2), 'u_init').contiguous()
        first_out, sets = self._ping_pong(B, obs.device)
        start = self.launches
        turn = [0]

        def step(u_nom, x_nom, gains, mu, need_gains):
            dest = first_out if gains is None else sets[turn[0]]
            if not need_gains:                                       # the last launch: no gains_out, so no backward sweep
                dest = {k: v for k, v in dest.items() if k != 'gains'}
            if gains is None:
                out = self._ilqr.launch(m, obs, u_nom, None, None, (), None, ri, pid, self._w5, dest)
            else:
                out = self._ilqr.launch(m, obs, u_nom, x_nom, gains, self._al, mu.contiguous(), ri, pid, self._w5, dest)
                turn[0] ^= 1
            self.launches += 1
            return out
        u, J_kernel, info = ilqr_loop(step, u0, self.iterations, self.mu0)
        return _finish(self, obs, u, J_kernel, info, ri, pid, start, 'ilqr')

    warm_start = staticmethod(OpenLoopMPC.warm_start)
