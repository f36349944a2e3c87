"""Closed-loop rollout of the analytic model under a policy with the per-step outputs: `steps` x [policy(obs) -> rollout_out].

The reference's drivers do this loop themselves — the shield for 5 steps (hier_decision.py:89-107), multi_ego's look-ahead for 20
(multi_ego.py:187-209) — and keep only a running penalty.  `policy_rollout` returns what a caller of the loop could have collected:
every step's five outputs, actions and states, the shield's sum and flag.

When the policy is this package's own `LoadPolicy` / `Policy4Toyota` with an fp16 `MLPNet`, and the pair fits the kernel
(include/envbuild_policy_rollout.h:eb_policy_rollout_supported), the whole horizon is ONE launch — policy and model step fused, the
rows never leaving the compute unit — and every array equals the loop's bit for bit.  Any other policy (an fp32 network, a callable)
runs the generic loop of `model.rollout_out(policy(model.obses))`.  Host glue only.

`policy_rollout_grad` is the training side: the same rollout under an fp32 network together with the gradient of its weighted cost with
respect to the network's parameters (include/envbuild_policy_rollout_grad.h) — three launches whatever the horizon where the pair fits
the kernel, the composed loop of the existing single entries elsewhere.

`policy_rollout_sample` is the stochastic side: `steps` x [eb_policy_sample -> eb_rollout_step] with every step's log-probability and
noise, and on request the reparameterised gradient of J = sum of cost + w_logp * sum of logp (include/envbuild_policy_rollout_sample.h)
— one launch forward-only, three with the parameter gradient.  Its four symbols are bound here on first use
(POLICY_ROLLOUT_SAMPLE_PROTOTYPES, `RolloutSampleArgs`): _capi's tables stay as they are."""
import ctypes as C

import torch

from . import _capi
from .dynamics_and_models import DevArray, _stream, _unwrap
from .shield import PENALTIES, _native_policy

WANT = ('out5', 'actions', 'obs')
GRAD_WANT = ('out5', 'actions', 'obs', 'cost', 'g_actions', 'g_obs0', 'g_params')


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


# ---- the rollout with its parameter gradient ----
def _net_of(policy, action_range):
    """(MLPNet, action_range) of a LoadPolicy / Policy4Toyota, or of a bare MLPNet with the action_range given"""
    from .policy import MLPNet
    if isinstance(policy, MLPNet):
        if policy.output_dim != 4:
            raise ValueError('the policy network must have 4 outputs (mean and log-std of two actions), got %d' % policy.output_dim)
        return policy, action_range
    native = _native_policy(policy)
    if native is None:
        raise ValueError('policy_rollout_grad needs an MLPNet / TrainableMLPNet or a LoadPolicy / Policy4Toyota with a deterministic policy')
    return native


def _w5(w5):
    w5 = [float(v) for v in w5]
    if len(w5) != 5:
        raise ValueError('w5 must hold the five weights of out5')
    return w5


def policy_rollout_grad(model, policy, obses, steps, w5, path_index=None, want=('cost', 'g_params'), ref_indexes=None, action_range=1.0,
                        fused=None):
    """The closed-loop rollout of `steps` steps under an fp32 network and the gradient of J = sum over envs of cost with respect to the
    network's parameters.  -> dict of DevArrays: 'obs' [B, D] (the state after the last step) and by `want` (a subset of GRAD_WANT)
    'out5_steps' [steps, 5, B], 'actions_steps' [steps, B, 2], 'obs_steps' [steps, B, D], 'cost' [B] (the sum over t of out5 weighted
    by w5, in include/envbuild_cand.h's order), 'g_actions_steps' [steps, B, 2], 'g_obs0' [B, 9], 'g_params' (flat, in
    Model.get_weights() order); 'fused' says whether eb_policy_rollout_grad ran.

    w5: five weights, also the cotangent of out5 at every step and env; ADP's loss is (-1, lam, 0, 0, 0) / (steps * B).
    `policy`: an MLPNet / TrainableMLPNet (its action head with `action_range`), or a LoadPolicy / Policy4Toyota.  `path_index` selects
    the path for a model in 'selecting' mode; a 'training'-mode model takes `ref_indexes` (or keeps its own).
    fused=None uses the one-call entry where eb_policy_rollout_grad_supported says yes and the composed loop of the existing entries
    (eb_policy_run_batch, eb_rollout_step, eb_rollout_step_vjp, eb_mlp_backward) elsewhere: the same arrays bit for bit, g_params as
    the float32 sum over t of the per-step gradients.  fused=True insists on the entry (a refused pair raises with the C reason),
    fused=False on the loop."""
    want = tuple(want)
    if any(w not in GRAD_WANT for w in want):
        raise ValueError('want must be a subset of %s' % (GRAD_WANT,))
    steps = int(steps)
    if steps < 1:
        raise ValueError('steps must be at least 1')
    w5 = _w5(w5)
    net, action_range = _net_of(policy, action_range)
    if path_index is not None:
        model.add_traj(obses, path_index)
    else:
        model.reset(obses, model.ref_indexes if ref_indexes is None else ref_indexes)
    if model.state_dtype != torch.float32:
        raise _capi.EbError("policy_rollout_grad: state_dtype='float16' has no reverse pass; use state_dtype='float32'")
    ar = -1.0 if action_range is None else float(action_range)
    if fused is None:
        ok = C.c_int32(0)
        model.api.policy_rollout_grad_supported(model.handle, net._handle, C.byref(ok))
        fused = bool(ok.value)
    out = (_fused_grad if fused else _composed_grad)(model, net, ar, steps, w5, want)
    model.obses = DevArray(out['obs'])
    model._after_tracking()
    return {k: (v if k == 'fused' else DevArray(v)) for k, v in out.items()}


_GRAD_NAMES = {'out5': 'out5_steps', 'actions': 'actions_steps', 'obs': 'obs_steps', 'cost': 'cost', 'g_actions': 'g_actions_steps',
               'g_obs0': 'g_obs0', 'g_params': 'g_params'}


def _param_count(model, net):
    count = C.c_int64(0)
    model.api.mlp_param_count(net._handle, C.byref(count))
    return count.value


def _fused_grad(model, net, ar, steps, w5, want):
    """one eb_policy_rollout_grad -> dict of tensors"""
    obs = _unwrap(model.obses).detach()
    B, D = obs.shape
    dev = model.device
    ri, pid = model._path_args()
    handle = net._handle
    need = C.c_size_t(0)
    model.api.policy_rollout_grad_workspace_bytes(model.handle, handle, B, steps, C.byref(need))
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    shapes = {'out5': (steps, 5, B), 'actions': (steps, B, 2), 'obs': (steps, B, D), 'cost': (B,), 'g_actions': (steps, B, 2),
              'g_obs0': (B, 9), 'g_params': (_param_count(model, net),)}
    bufs = {k: (f32(*shapes[k]) if k in want else None) for k in GRAD_WANT}
    obs_out = torch.empty_like(obs)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    model.api.policy_rollout_grad(model.handle, handle, B, steps, p(obs), p(ri), pid, C.c_float(ar), (C.c_float * 5)(*w5), p(ws), need.value,
                                  p(obs_out), *[p(bufs[k]) for k in GRAD_WANT], _stream(dev))
    out = {'fused': True, 'obs': obs_out}
    out.update({_GRAD_NAMES[k]: v for k, v in bufs.items() if v is not None})
    return out


def _composed_grad(model, net, ar, steps, w5, want):
    """the loop of existing entries the one-call form is held to: forward `steps` x [eb_policy_run_batch -> eb_rollout_step], then for
    t = steps - 1 .. 0 eb_rollout_step_vjp and eb_mlp_backward, lambda_t = s_t[:, :9] + p_t[:, :9]"""
    api = model.api
    obs = _unwrap(model.obses).detach()
    B, D = obs.shape
    dev = model.device
    ri, pid = model._path_args()
    handle = net._handle
    stream = _stream(dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    pre, acts, out5 = f32(steps + 1, B, D), f32(steps, B, 2), f32(steps, 5, B)
    pre[0] = obs
    scaled = f32(B, 2)
    for t in range(steps):
        api.policy_run_batch(handle, B, p(pre[t]), C.c_float(ar), p(acts[t]), stream)
        api.rollout_step(model.handle, B, p(pre[t]), p(acts[t]), p(ri), pid, p(pre[t + 1]), p(out5[t]), p(scaled), stream)
    need = C.c_size_t(0)
    api.mlp_backward_workspace_bytes(handle, B, C.byref(need))
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    g5 = torch.tensor(w5, dtype=torch.float32, device=dev).view(5, 1).expand(5, B).contiguous()
    lam, s, pt, g_act = torch.zeros((B, 9), dtype=torch.float32, device=dev), f32(B, 9), f32(B, D), f32(steps, B, 2)
    g_step = f32(_param_count(model, net)) if 'g_params' in want else None
    g_par = torch.zeros_like(g_step) if g_step is not None else None
    vjp = api.grad_fn('eb_rollout_step_vjp')
    for t in range(steps - 1, -1, -1):
        api.check(vjp(model.handle, B, p(pre[t]), p(acts[t]), p(ri), pid, p(lam), 9, p(g5), p(s), 9, p(g_act[t]), stream))
        api.mlp_backward(handle, B, p(pre[t]), p(g_act[t]), 1, C.c_float(ar), p(ws), need.value, None, p(pt), p(g_step), stream)
        lam = s + pt[:, :9]
        if g_par is not None:
            g_par = g_par + g_step
    out = {'fused': False, 'obs': pre[steps].clone()}
    if 'cost' in want:          # include/envbuild_cand.h: s_t = the rows with a non-zero weight in row order, J = ascending t from +0
        rows = [r for r in range(5) if w5[r] != 0.0]
        J = torch.zeros((B,), dtype=torch.float32, device=dev)
        for t in range(steps if rows else 0):
            st = None
            for r in rows:
                term = out5[t, r] * w5[r]
                st = term if st is None else st + term
            J = J + st
        out['cost'] = J
    given = {'out5': out5, 'actions': acts, 'obs': pre[1:], 'g_actions': g_act, 'g_obs0': lam, 'g_params': g_par}
    out.update({_GRAD_NAMES[k]: given[k] for k in want if k != 'cost'})
    return out


# ---- the stochastic rollout with its reparameterised gradient (include/envbuild_policy_rollout_sample.h) ----
EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION = 1
POLICY_ROLLOUT_SAMPLE_MAX_STEPS = 128
SAMPLE_HEADER = 'envbuild_policy_rollout_sample.h'
_P, _I, _F = C.c_void_p, C.c_int32, C.c_float


class RolloutSampleArgs(C.Structure):
    """eb_policy_rollout_sample_args, field for field"""
    _fields_ = [('struct_size', C.c_uint32), ('n_env', _I), ('steps', _I), ('path_id', _I), ('action_range', _F), ('w_logp', _F),
                ('w5', _F * 5), ('seed', C.c_uint64), ('counter', C.c_uint64), ('obs_in', _P), ('ref_idx', _P), ('row_ids', _P),
                ('eps_steps', _P), ('workspace', _P), ('workspace_bytes', C.c_size_t), ('obs_out', _P), ('out5_steps', _P),
                ('actions_steps', _P), ('obs_steps', _P), ('cost', _P), ('logp_steps', _P), ('eps_out_steps', _P),
                ('g_actions_steps', _P), ('g_obs0', _P), ('g_params', _P), ('stream', _P)]


# name -> (restype, argtypes) for every symbol the header declares
POLICY_ROLLOUT_SAMPLE_PROTOTYPES = {
    'eb_policy_rollout_sample_abi_version': (C.c_int, []),
    'eb_policy_rollout_sample_supported': (C.c_int, [_P, _P, C.POINTER(_I)]),
    # (h, policy, n_env, steps, with_grad, bytes)
    'eb_policy_rollout_sample_workspace_bytes': (C.c_int, [_P, _P, _I, _I, _I, C.POINTER(C.c_size_t)]),
    'eb_policy_rollout_sample': (C.c_int, [_P, _P, C.POINTER(RolloutSampleArgs)]),
}
SAMPLE_WANT = ('out5', 'actions', 'obs', 'cost', 'logp', 'eps', 'g_actions', 'g_obs0', 'g_params')
_SAMPLE_NAMES = dict(_GRAD_NAMES, logp='logp_steps', eps='eps_steps')
_SAMPLE_FIELDS = {'out5': 'out5_steps', 'actions': 'actions_steps', 'obs': 'obs_steps', 'cost': 'cost', 'logp': 'logp_steps',
                  'eps': 'eps_out_steps', 'g_actions': 'g_actions_steps', 'g_obs0': 'g_obs0', 'g_params': 'g_params'}


def bind_sample(api):
    """name -> raw ctypes function for every entry of POLICY_ROLLOUT_SAMPLE_PROTOTYPES on `api` (a _capi.CApi), bound on first use;
    EbError when the library does not export them or speaks another version."""
    fns = api.__dict__.setdefault('_policy_rollout_sample_fns', {})
    if not fns:
        missing = [n for n in POLICY_ROLLOUT_SAMPLE_PROTOTYPES if not hasattr(api.lib, n)]
        if missing:
            raise _capi.EbError('%s (backend %r) does not export %s: this library has no stochastic closed-loop rollout (include/%s is '
                                'implemented by the HIP library only; rebuild an older one)'
                                % (api.path, api.backend, ', '.join(missing), SAMPLE_HEADER))
        for n, (res, args) in POLICY_ROLLOUT_SAMPLE_PROTOTYPES.items():
            fn = getattr(api.lib, n)
            fn.restype, fn.argtypes = res, args
            fns[n] = fn
        v = fns['eb_policy_rollout_sample_abi_version']()
        if v != EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION:
            fns.clear()
            raise _capi.EbError('%s: policy-rollout-sample ABI version %d, expected %d (include/%s)'
                                % (api.path, v, EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION, SAMPLE_HEADER))
    return fns


def sample_args(**fields):
    """a RolloutSampleArgs with struct_size set, everything else zero / NULL unless given (w5: five floats)"""
    a = RolloutSampleArgs()
    a.struct_size = C.sizeof(RolloutSampleArgs)
    for k, v in fields.items():
        if k == 'w5':
            a.w5 = (_F * 5)(*[float(x) for x in v])
        else:
            setattr(a, k, v)
    return a


def _sample_call(api, name, *args):
    api.check(bind_sample(api)[name](*args))


def policy_rollout_sample(model, policy, obses, steps, w5=None, w_logp=0.0, path_index=None, action_range=1.0, eps=None, seed=0, counter=0,
                          row_ids=None, want=('actions', 'logp'), ref_indexes=None, fused=None):
    """The closed-loop rollout of `steps` steps under the STOCHASTIC head of an fp32 or fp16 network: step t samples
    a_t ~ action_range * tanh(N(mean, exp(log_std))) with (seed, counter + t) — or takes eps [steps, B, 2] as the noise — and steps the
    model.  -> dict of DevArrays: 'obs' [B, D] (the state after the last step) and by `want` (a subset of SAMPLE_WANT) 'out5_steps'
    [steps, 5, B], 'actions_steps' [steps, B, 2], 'obs_steps' [steps, B, D], 'cost' [B] (w5's weighted sum, include/envbuild_cand.h's
    order; logp is not folded in), 'logp_steps' [steps, B], 'eps_steps' [steps, B, 2] (the noise used), and the reparameterised gradient
    of J = sum of cost + w_logp * sum of logp: 'g_actions_steps' [steps, B, 2], 'g_obs0' [B, 9], 'g_params' (flat); 'fused' says
    whether eb_policy_rollout_sample ran.

    w5 None: zeros (no cost, no cost gradient).  row_ids [B] (unsigned 32-bit numbers, None: the row index) name the rows' draws.
    fused=None uses the one-call entry where eb_policy_rollout_sample_supported says yes and the composed loop of the existing entries
    (eb_policy_sample or eb_mlp_forward + eb_policy_sample_from_logits, eb_rollout_step, eb_rollout_step_vjp, eb_policy_sample_vjp,
    eb_mlp_backward) elsewhere — an fp16 MLPNet, a wide network, n_veh 64: the same per-row arrays, g_params as the float32 sum over t
    of the per-step gradients; on that route a gradient of an fp16 handle is refused as eb_mlp_backward refuses it.  fused=True
    insists on the entry (a refused pair raises with the C reason), fused=False on the loop."""
    from . import policy_sample as _ps
    want = tuple(want)
    if any(w not in SAMPLE_WANT for w in want):
        raise ValueError('want must be a subset of %s' % (SAMPLE_WANT,))
    steps = int(steps)
    if steps < 1:
        raise ValueError('steps must be at least 1')
    w5 = _w5((0.0,) * 5 if w5 is None else w5)
    net, action_range = _net_of(policy, action_range)
    ar = _ps._range(action_range)
    if path_index is not None:
        model.add_traj(obses, path_index)
    else:
        model.reset(obses, model.ref_indexes if ref_indexes is None else ref_indexes)
    if model.state_dtype != torch.float32:
        raise _capi.EbError("policy_rollout_sample: state_dtype='float16' is not supported; use state_dtype='float32'")
    B = _unwrap(model.obses).shape[0]
    e = None
    if eps is not None:
        e = _unwrap(eps)
        e = (e if isinstance(e, torch.Tensor) else torch.as_tensor(e)).detach().to(device=model.device, dtype=torch.float32).contiguous()
        if tuple(e.shape) != (steps, B, 2):
            raise ValueError('eps must be [%d, %d, 2], got %s' % (steps, B, tuple(e.shape)))
    ids = _ps._row_ids(row_ids, B, model.device)
    if fused is None:
        ok = C.c_int32(0)
        _sample_call(model.api, 'eb_policy_rollout_sample_supported', model.handle, net._handle, C.byref(ok))
        fused = bool(ok.value)
    run = _fused_sample if fused else _composed_sample
    out = run(model, net, ar, steps, w5, float(w_logp), e, int(seed), int(counter), ids, want)
    model.obses = DevArray(out['obs'])
    model._after_tracking()
    return {k: (v if k == 'fused' else DevArray(v)) for k, v in out.items()}


def _fused_sample(model, net, ar, steps, w5, w_logp, eps, seed, counter, ids, want, stream=None):
    """one eb_policy_rollout_sample -> dict of tensors"""
    obs = _unwrap(model.obses).detach()
    B, D = obs.shape
    dev = model.device
    ri, pid = model._path_args()
    with_grad = any(k in want for k in ('g_actions', 'g_obs0', 'g_params'))
    need = C.c_size_t(0)
    _sample_call(model.api, 'eb_policy_rollout_sample_workspace_bytes', model.handle, net._handle, B, steps, int(with_grad), C.byref(need))
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev) if need.value else None
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    shapes = {'out5': (steps, 5, B), 'actions': (steps, B, 2), 'obs': (steps, B, D), 'cost': (B,), 'logp': (steps, B), 'eps': (steps, B, 2),
              'g_actions': (steps, B, 2), 'g_obs0': (B, 9), 'g_params': (_param_count(model, net),)}
    bufs = {k: (f32(*shapes[k]) if k in want else None) for k in SAMPLE_WANT}
    obs_out = torch.empty_like(obs)
    p = lambda t: t.data_ptr() if t is not None else None
    a = sample_args(n_env=B, steps=steps, path_id=pid, action_range=ar, w_logp=w_logp, w5=w5, seed=seed % 2 ** 64, counter=counter % 2 ** 64,
                    obs_in=p(obs), ref_idx=p(ri), row_ids=p(ids), eps_steps=p(eps), workspace=p(ws), workspace_bytes=need.value,
                    obs_out=p(obs_out), stream=_stream(dev) if stream is None else stream,
                    **{_SAMPLE_FIELDS[k]: p(v) for k, v in bufs.items()})
    _sample_call(model.api, 'eb_policy_rollout_sample', model.handle, net._handle, C.byref(a))
    out = {'fused': True, 'obs': obs_out}
    out.update({_SAMPLE_NAMES[k]: v for k, v in bufs.items() if v is not None})
    return out


def _composed_sample(model, net, ar, steps, w5, w_logp, eps, seed, counter, ids, want):
    """the loop of existing entries the one-call form is held to (include/envbuild_policy_rollout_sample.h states it)"""
    from . import policy_sample as _ps
    from .policy import MLPNet
    api = model.api
    obs = _unwrap(model.obses).detach()
    B, D = obs.shape
    dev = model.device
    ri, pid = model._path_args()
    handle = net._handle
    stream = _stream(dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    with_grad = any(k in want for k in ('g_actions', 'g_obs0', 'g_params'))
    one_launch = _ps._supported(net)
    if with_grad and not one_launch:
        api.check(-1)                                        # eb_policy_sample_supported's reason: an fp16 handle has no gradient
    pre, acts, out5 = f32(steps + 1, B, D), f32(steps, B, 2), f32(steps, 5, B)
    logp, used, ys = f32(steps, B), f32(steps, B, 2), f32(steps, B, 4)
    pre[0] = obs
    scaled = f32(B, 2)
    for t in range(steps):
        out = {'actions': acts[t], 'logp': logp[t], 'eps': used[t], 'logits': ys[t]}
        if one_launch:
            _ps._fused(net, pre[t], ar, None if eps is None else eps[t], seed, counter + t, ids, out)
        else:
            y = _unwrap(MLPNet.call(net, DevArray(pre[t]))).to(torch.float32).contiguous()
            ys[t] = y
            _ps._from_logits(api, y, ar, None if eps is None else eps[t], seed, counter + t, ids, out)
        api.rollout_step(model.handle, B, p(pre[t]), p(acts[t]), p(ri), pid, p(pre[t + 1]), p(out5[t]), p(scaled), stream)
    given = {'out5': out5, 'actions': acts, 'obs': pre[1:], 'logp': logp, 'eps': used}
    if with_grad:
        need = C.c_size_t(0)
        api.mlp_backward_workspace_bytes(handle, B, C.byref(need))
        ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
        g5 = torch.tensor(w5, dtype=torch.float32, device=dev).view(5, 1).expand(5, B).contiguous()
        g_lp = torch.full((B,), w_logp, dtype=torch.float32, device=dev)
        lam, s, pt, g_act, g_y = torch.zeros((B, 9), dtype=torch.float32, device=dev), f32(B, 9), f32(B, D), f32(steps, B, 2), f32(B, 4)
        g_step = f32(_param_count(model, net)) if 'g_params' in want else None
        g_par = torch.zeros_like(g_step) if g_step is not None else None
        vjp = api.grad_fn('eb_rollout_step_vjp')
        for t in range(steps - 1, -1, -1):
            api.check(vjp(model.handle, B, p(pre[t]), p(acts[t]), p(ri), pid, p(lam), 9, p(g5), p(s), 9, p(g_act[t]), stream))
            _ps._call(api, 'eb_policy_sample_vjp', B, 4, ys[t].data_ptr(), used[t].data_ptr(), ar, g_act[t].data_ptr(), g_lp.data_ptr(),
                      g_y.data_ptr(), stream)
            api.mlp_backward(handle, B, p(pre[t]), p(g_y), 0, C.c_float(0.0), p(ws), need.value, None, p(pt), p(g_step), stream)
            lam = s + pt[:, :9]
            if g_par is not None:
                g_par = g_par + g_step
        given.update({'g_actions': g_act, 'g_obs0': lam, 'g_params': g_par})
    out = {'fused': False, 'obs': pre[steps].clone()}
    if 'cost' in want:          # include/envbuild_cand.h: s_t = the rows with a non-zero weight in row order, J = ascending t from +0
        rows = [r for r in range(5) if w5[r] != 0.0]
        J = torch.zeros((B,), dtype=torch.float32, device=dev)
        for t in range(steps if rows else 0):
            st = None
            for r in rows:
                term = out5[t, r] * w5[r]
                st = term if st is None else st + term
            J = J + st
        out['cost'] = J
    out.update({_SAMPLE_NAMES[k]: given[k] for k in want if k != 'cost'})
    return out
