"""Gradients through the model rollout: EnvironmentModel.rollout_out on the torch.autograd graph.

The reference's analytic model is differentiable on purpose — model-based RL back-propagates the rollout's sum of `rewards` and
`punish_term_for_training` into the policy (DAM:118-126, with tf.stop_gradient on the vehicle columns, DAM:195, 331, 402).  Here the
forward of one step is the eb_rollout_step launch EnvironmentModel uses, and its backward is one eb_rollout_step_vjp launch
(include/envbuild_grad.h, csrc/eb_rollout_vjp.hip) on the current stream, recomputing from the saved pre-step obs and raw actions.

    model = DifferentiableEnvironmentModel('left', mode='training')
    model.reset(obses, ref_indexes)                      # torch tensors; obses [B, D] may itself require grad
    for _ in range(25):
        obses, rewards, punish, *_ = model.rollout_out(policy(obses))
        loss = loss + (-rewards + 10. * punish).mean()
    loss.backward()                                      # into the policy's parameters

The gradient contract is the header's: obs[:, :nd] and the raw actions receive a gradient, the vehicle columns exactly zero; clipped
actions (beyond +-1.05) and a clipped v_x get zero; the closest path point is a constant.  fp32 state only: there is no reverse
pass for state_dtype='float16'.  No CPU path and no fall-back to eager PyTorch: without the HIP library's reverse pass this raises.

An open-loop rollout over a whole action tape — an MPC cost — is the free function rollout_tape(model, obses, action_tape): forward one
eb_rollout_tape launch, backward one eb_rollout_tape_vjp launch (csrc/eb_rollout_tape_vjp.hip).
"""
import torch

from . import _capi
from ._tape_args import check_rows, need_fp32
from .dynamics_and_models import EnvironmentModel, DevArray, _dev, _stream, _unwrap

__all__ = ['DifferentiableEnvironmentModel', 'rollout_step', 'rollout_tape', 'tape_vjp_max_horizon']


class _RolloutStep(torch.autograd.Function):
    """(obs [B, D], raw actions [B, 2]) -> (next obs [B, D], out5 [5, B], scaled actions [B, 2]) of one model step."""

    @staticmethod
    def forward(ctx, obs, actions, model, ref_idx, path_id):
        B = obs.shape[0]
        obs_out = torch.empty_like(obs)
        out7 = torch.empty((7, B), dtype=torch.float32, device=obs.device)     # out5 rows | scaled actions, as EnvironmentModel lays them out
        rc = model.api.lib.eb_rollout_step(model.handle, B, obs.data_ptr(), actions.data_ptr(),
                                           None if ref_idx is None else ref_idx.data_ptr(), path_id, obs_out.data_ptr(),
                                           out7.data_ptr(), out7.data_ptr() + 5 * B * 4, _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        ctx.save_for_backward(obs, actions)
        ctx.model, ctx.ref_idx, ctx.path_id = model, ref_idx, path_id
        ctx.set_materialize_grads(False)          # an unused output's cotangent arrives as None -> NULL = zeros, no zero tensor made
        scaled = out7[5:].view(B, 2)
        ctx.mark_non_differentiable(scaled)
        return obs_out, out7[:5], scaled

    @staticmethod
    def backward(ctx, g_obs_out, g_out5, _g_scaled):
        obs, actions = ctx.saved_tensors
        model = ctx.model
        B, D = obs.shape
        if g_obs_out is not None:
            g_obs_out = g_obs_out.contiguous()
        if g_out5 is not None:
            g_out5 = g_out5.contiguous()
        g_obs = torch.empty_like(obs)             # full rows: the launch zero-fills the vehicle columns
        g_act = torch.empty_like(actions)
        rc = model._vjp_fn(model.handle, B, obs.data_ptr(), actions.data_ptr(),
                           None if ctx.ref_idx is None else ctx.ref_idx.data_ptr(), ctx.path_id,
                           None if g_obs_out is None else g_obs_out.data_ptr(), D,
                           None if g_out5 is None else g_out5.data_ptr(), g_obs.data_ptr(), D, g_act.data_ptr(),
                           _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        return g_obs, g_act, None, None, None


def _graph_tensor(x, device, what):
    """a float32 contiguous tensor on `device` that is still attached to x's graph"""
    x = _unwrap(x)
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(x)
    return x.to(device=device, dtype=torch.float32).contiguous()


def rollout_step(model, obses, actions):
    """One differentiable model step at an explicit state: -> (next obses [B, D], out5 [5, B]).  `model` supplies the task, the slot
    modes and the path choice (reset / add_traj); its own state is not touched."""
    obs = model._obs_graph(obses)
    act = _graph_tensor(actions, model.device, 'actions')
    ri, pid = model._path_args()
    nxt, out5, _ = _RolloutStep.apply(obs, act, model, ri, pid)
    return nxt, out5


class _RolloutTape(torch.autograd.Function):
    """(obs [B, D], raw tape [H, B, 2]) -> (final obs [B, D], out5 [H, 5, B]): forward one eb_rollout_tape launch, backward one
    eb_rollout_tape_vjp launch that recomputes from obs and the tape (nothing else is saved)."""

    @staticmethod
    def forward(ctx, obs, tape, model, ref_idx, path_id):
        H, B = tape.shape[0], obs.shape[0]
        work, out = torch.empty_like(obs), torch.empty_like(obs)
        out5 = torch.empty((H, 5, B), dtype=torch.float32, device=obs.device)
        rc = model.api.lib.eb_rollout_tape(model.handle, B, H, obs.data_ptr(), tape.data_ptr(),
                                           None if ref_idx is None else ref_idx.data_ptr(), path_id, work.data_ptr(), out.data_ptr(),
                                           out5.data_ptr(), _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        ctx.save_for_backward(obs, tape)
        ctx.model, ctx.ref_idx, ctx.path_id = model, ref_idx, path_id
        ctx.set_materialize_grads(False)
        return out, out5

    @staticmethod
    def backward(ctx, g_final, g_out5):
        obs, tape = ctx.saved_tensors
        model = ctx.model
        H, (B, D) = tape.shape[0], obs.shape
        nd = D - 4 * model.veh_num
        if g_final is not None:
            g_final = g_final.contiguous()
        if g_out5 is not None:
            g_out5 = g_out5.contiguous()
        g_obs = torch.zeros_like(obs)             # the vehicle columns stay exact zeros (stop_gradient)
        g_head = torch.empty((B, nd), dtype=torch.float32, device=obs.device)
        g_tape = torch.empty_like(tape)
        rc = model.api.grad_fn('eb_rollout_tape_vjp')(
            model.handle, B, H, obs.data_ptr(), tape.data_ptr(), None if ctx.ref_idx is None else ctx.ref_idx.data_ptr(), ctx.path_id,
            None if g_final is None else g_final.data_ptr(), D, None if g_out5 is None else g_out5.data_ptr(), None, None, None,
            g_head.data_ptr(), g_tape.data_ptr(), _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        g_obs[:, :nd] = g_head
        return g_obs, g_tape, None, None, None


class _RolloutTapeComposed(torch.autograd.Function):
    """The same pair for a horizon beyond eb_rollout_tape_vjp_max_horizon: H eb_rollout_step launches that keep every pre-step
    obs, and eb_rollout_chain_vjp (H reverse launches) backwards."""

    @staticmethod
    def forward(ctx, obs, tape, model, ref_idx, path_id):
        H, (B, D) = tape.shape[0], obs.shape
        steps = torch.empty((H + 1, B, D), dtype=torch.float32, device=obs.device)
        steps[0] = obs
        out5 = torch.empty((H, 5, B), dtype=torch.float32, device=obs.device)
        scaled = torch.empty((B, 2), dtype=torch.float32, device=obs.device)
        for t in range(H):
            rc = model.api.lib.eb_rollout_step(model.handle, B, steps[t].data_ptr(), tape[t].data_ptr(),
                                               None if ref_idx is None else ref_idx.data_ptr(), path_id, steps[t + 1].data_ptr(),
                                               out5[t].data_ptr(), scaled.data_ptr(), _stream(model.device))
            if rc != 0:
                model.api.check(rc)
        ctx.save_for_backward(steps, tape)
        ctx.model, ctx.ref_idx, ctx.path_id = model, ref_idx, path_id
        ctx.set_materialize_grads(False)
        return steps[H].clone(), out5

    @staticmethod
    def backward(ctx, g_final, g_out5):
        steps, tape = ctx.saved_tensors
        model = ctx.model
        H, B, D = tape.shape[0], steps.shape[1], steps.shape[2]
        nd = D - 4 * model.veh_num
        if g_final is not None:
            g_final = g_final.contiguous()
        if g_out5 is not None:
            g_out5 = g_out5.contiguous()
        g_obs = torch.zeros((B, D), dtype=torch.float32, device=steps.device)
        work, g_head = (torch.empty((B, nd), dtype=torch.float32, device=steps.device) for _ in range(2))
        g_tape = torch.empty_like(tape)
        rc = model.api.grad_fn('eb_rollout_chain_vjp')(
            model.handle, B, H, steps.data_ptr(), tape.data_ptr(), None if ctx.ref_idx is None else ctx.ref_idx.data_ptr(), ctx.path_id,
            None if g_final is None else g_final.data_ptr(), D, None if g_out5 is None else g_out5.data_ptr(), work.data_ptr(),
            g_head.data_ptr(), g_tape.data_ptr(), _stream(model.device))
        if rc != 0:
            model.api.check(rc)
        g_obs[:, :nd] = g_head
        return g_obs, g_tape, None, None, None


def tape_vjp_max_horizon(model):
    """the longest tape eb_rollout_tape_vjp takes for `model` (its slot count decides)"""
    import ctypes
    limit = ctypes.c_int32(0)
    model.api.check(model.api.grad_fn('eb_rollout_tape_vjp_max_horizon')(model.handle, ctypes.byref(limit)))
    return limit.value


def rollout_tape(model, obses, action_tape):
    """A differentiable open-loop rollout at an explicit state: -> (final obses [B, D], out5_steps [H, 5, B]) on the autograd graph.
    Forward is one eb_rollout_tape launch, backward one eb_rollout_tape_vjp launch that recomputes from `obses` and the tape;
    obses[:, :nd] and the tape receive gradients, the vehicle columns exact zeros.  `model` (an EnvironmentModel with fp32 state)
    supplies the task, the slot modes and the path choice; its own state is not touched.  A tape longer than
    tape_vjp_max_horizon(model) falls back to H step launches that keep every pre-step obs plus eb_rollout_chain_vjp — the same
    bits, 2 H launches."""
    need_fp32(model, 'grad.rollout_tape: fp32 state only (the fp16-state kernels have no reverse pass)')
    obs = check_rows(model, _graph_tensor(obses, model.device, 'obses'))
    tape = _graph_tensor(action_tape, model.device, 'action_tape')
    if tape.dim() != 3 or tape.shape[1] != obs.shape[0] or tape.shape[2] != 2 or tape.shape[0] < 1:
        raise ValueError('action_tape must be [H, %d, 2]; got %s' % (obs.shape[0], tuple(tape.shape)))
    ri, pid = model._path_args()
    fn = _RolloutTape if tape.shape[0] <= tape_vjp_max_horizon(model) else _RolloutTapeComposed
    return fn.apply(obs, tape, model, ri, pid)


class DifferentiableEnvironmentModel(EnvironmentModel):
    """EnvironmentModel (DAM:90-427) whose reset / add_traj / rollout_out take and return torch.Tensors on the autograd graph.
    `obses` is full width [B, D]; the vehicle columns of its gradient are zero.  Everything else is inherited unchanged."""

    def __init__(self, training_task, num_future_data=0, mode='training', n_veh=None, device=None, state_dtype='float32'):
        if state_dtype != 'float32':
            raise _capi.EbError("DifferentiableEnvironmentModel: state_dtype=%r has no reverse pass — the fp16-state kernels "
                                "(eb_rollout_step_f16) are forward only; use state_dtype='float32'" % (state_dtype,))
        EnvironmentModel.__init__(self, training_task, num_future_data, mode=mode, n_veh=n_veh, device=device,
                                  state_dtype='float32', copy_outputs=True)
        self._vjp_fn = self.api.grad_fn('eb_rollout_step_vjp')     # EbError here, not at the first backward(), when the library has none

    def _obs_graph(self, obses):
        t = _graph_tensor(obses, self.device, 'obses')
        if t.dim() != 2 or t.shape[1] != self.obs_dim:
            raise ValueError('obses must be [B, %d] for task=%s, n_veh=%d, num_future_data=%d; got %s'
                             % (self.obs_dim, self.task, self.veh_num, self.num_future_data, tuple(t.shape)))
        return t

    def reset(self, obses, ref_indexes=None):  # DAM:108-112
        self.obses = self._obs_graph(obses)
        self.ref_indexes = ref_indexes
        self._ref_idx_dev = None if ref_indexes is None else _dev(ref_indexes, self.device, torch.int32)
        self.actions = None
        self.reward_info = None

    def add_traj(self, obses, path_index):  # DAM:114-116
        self.obses = self._obs_graph(obses)
        self.ref_path.set_path(path_index)

    def rollout_out(self, actions):  # DAM:118-126
        """-> (obses, rewards, punish_term_for_training, real_punish_term, veh2veh4real, veh2road4real): torch tensors on the graph."""
        obs = self._obs_graph(self.obses)
        act = _graph_tensor(actions, self.device, 'actions')
        ri, pid = self._path_args()
        nxt, out5, scaled = _RolloutStep.apply(obs, act, self, ri, pid)
        self.obses = nxt
        self.actions = DevArray(scaled)
        self._after_tracking()
        return nxt, out5[0], out5[1], out5[2], out5[3], out5[4]

    def rollout_tape(self, action_tape):
        raise _capi.EbError('DifferentiableEnvironmentModel.rollout_tape: the open-loop tape kernel has no reverse pass; loop over '
                            'rollout_out, or use EnvironmentModel for a forward-only rollout')   # (differentiable: grad.rollout_tape)
