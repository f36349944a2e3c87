"""Closed-loop rollout of the analytic model under a policy with the per-step outputs: `steps` x [policy(obs) -> rollout_out].

The reference's drivers do this loop themselves — the shield for 5 steps (hier_decision.py:89-107), multi_ego's look-ahead for 20
(multi_ego.py:187-209) — and keep only a running penalty.  `policy_rollout` returns what a caller of the loop could have collected:
every step's five outputs, actions and states, the shield's sum and flag.

When the policy is this package's own `LoadPolicy` / `Policy4Toyota` with an fp16 `MLPNet`, and the pair fits the kernel
(include/envbuild_policy_rollout.h:eb_policy_rollout_supported), the whole horizon is ONE launch — policy and model step fused, the
rows never leaving the compute unit — and every array equals the loop's bit for bit.  Any other policy (an fp32 network, a callable)
runs the generic loop of `model.rollout_out(policy(model.obses))`.  Host glue only."""
import ctypes as C

import torch

from . import _capi
from .dynamics_and_models import DevArray, _stream, _unwrap
from .shield import PENALTIES, _native_policy

WANT = ('out5', 'actions', 'obs')


def _fused_pair(model, policy):
    """(MLPNet, action_range) when eb_policy_rollout takes this model and policy, else None."""
    native = _native_policy(policy)
    if native is None or model.state_dtype != torch.float32 or native[0].device != model.device:
        return None
    ok = C.c_int32(0)
    model.api.policy_rollout_supported(model.handle, native[0]._handle, C.byref(ok))
    return native if ok.value else None


def fused_is_safe(model, policy, obses, steps, path_index, penalty):
    """shield.is_safe(fused=True): (safe, punish) through the one-launch kernel, or None when the pair does not fit it (the caller goes on as without `fused`)"""
    if _native_policy(policy) is None:
        return None
    if path_index is not None:
        model.add_traj(obses, path_index)
    else:
        model.reset(obses, model.ref_indexes)
    native = _fused_pair(model, policy)
    if native is None:
        return None
    out = _fused(model, native, steps, penalty, ())
    return out['safe'], out['punish']


def policy_rollout(model, policy, obses, steps, path_index=None, penalty='veh2veh4real', want=('out5',)):
    """-> dict of DevArrays: 'obs' [B, D] (the state after the last step), 'punish' [B], 'safe' [B] bool, and by `want` (a subset of
    ('out5', 'actions', 'obs')) 'out5_steps' [steps, 5, B], 'actions_steps' [steps, B, 2], 'obs_steps' [steps, B, D] (the state AFTER
    step t); 'fused' (a bool) says whether the one-launch kernel ran.  `path_index` selects the path for a model in 'selecting' mode; a
    'training'-mode model keeps its ref_indexes.  Leaves model.obses where the loop of rollout_out calls would."""
    if penalty not in PENALTIES:
        raise ValueError('penalty must be one of %s' % sorted(PENALTIES))
    want = tuple(want)
    if any(w not in WANT for w in want):
        raise ValueError('want must be a subset of %s' % (WANT,))
    steps = int(steps)
    if steps < 1:
        raise ValueError('steps must be at least 1')
    if path_index is not None:
        model.add_traj(obses, path_index)
    else:
        model.reset(obses, model.ref_indexes)
    native = _fused_pair(model, policy)
    if native is not None:
        return _fused(model, native, steps, penalty, want)
    out = {'fused': False}
    out5s, acts, obss = [], [], []
    punish = None
    head = _native_policy(policy)          # a LoadPolicy / Policy4Toyota the kernel does not take: its deterministic action
    run = policy if head is None else (lambda o: head[0].mode(o, head[1]))
    for _ in range(steps):
        a = run(model.obses)
        r = model.rollout_out(a)
        p = _unwrap(r[PENALTIES[penalty]])
        punish = p.clone() if punish is None else punish + p
        if 'out5' in want:
            out5s.append(torch.stack([_unwrap(x).to(torch.float32) for x in r[1:6]]))
        if 'actions' in want:
            acts.append(_unwrap(a).to(device=model.device, dtype=torch.float32).clone())
        if 'obs' in want:
            obss.append(_unwrap(model.obses).clone())
    out['obs'] = DevArray(_unwrap(model.obses))
    if 'out5' in want:
        out['out5_steps'] = DevArray(torch.stack(out5s))
    if 'actions' in want:
        out['actions_steps'] = DevArray(torch.stack(acts))
    if 'obs' in want:
        out['obs_steps'] = DevArray(torch.stack(obss))
    out['punish'] = DevArray(punish)
    out['safe'] = DevArray(~(punish > 0))
    return out


def _fused(model, native, steps, penalty, want):
    net, action_range = native
    obs = _unwrap(model.obses)
    B, D = obs.shape
    dev = model.device
    ri, pid = model._path_args()
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    obs_out = torch.empty_like(obs)
    out5 = f32(steps, 5, B) if 'out5' in want else None
    acts = f32(steps, B, 2) if 'actions' in want else None
    obss = f32(steps, B, D) if 'obs' in want else None
    punish = f32(B)
    safe = torch.empty((B,), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    model.api.policy_rollout(model.handle, net._handle, B, steps, p(obs), p(ri), pid,
                             C.c_float(-1.0 if action_range is None else float(action_range)), _capi.PENALTY_ID[penalty],
                             p(obs_out), p(out5), p(acts), p(obss), p(punish), p(safe), _stream(dev))
    model.obses = DevArray(obs_out)
    model._after_tracking()
    out = {'fused': True, 'obs': DevArray(obs_out)}
    if out5 is not None:
        out['out5_steps'] = DevArray(out5)
    if acts is not None:
        out['actions_steps'] = DevArray(acts)
    if obss is not None:
        out['obs_steps'] = DevArray(obss)
    out['punish'] = DevArray(punish)
    out['safe'] = DevArray(safe.bool())
    return out
