#!/usr/bin/env python3
"""Profiling aid: the policy network's backward (csrc/eb_policy_grad.hip, include/envbuild_mlp_grad.h) against a plain torch twin, and
the device-side weight set against `set_weights` through the host, in ONE process on cuda:0, HIP events on the launch stream,
alternating windows, the discipline of scripts/time_policy_f16.py:

  (backward)  one eb_mlp_backward with all three outputs at 65 536 x (137 -> 256 -> 256 -> 4), elu hidden, linear out, scale set,
              against the torch twin's fp32 forward + backward (torch.nn.Sequential of the same layers, gradients to the input and to
              every parameter);
  (small)     the same at 4 096 x (41 -> 256 -> 256 -> 4);
  (weights)   eb_mlp_set_params_device from the flat device tensor against MLPNet.set_weights (host arrays, a new handle, a sync).

No bar is attached: the entries are written with their window spreads and `faster` names the side with the lower median.

Every GPU step of a job that calls this runs under its own `timeout`.

    python scripts/time_policy_grad.py [--iters 20] [--windows 5] [--out FILE]"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from env_build_amd.dynamics_and_models import _stream
from env_build_amd.policy import MLPNet
from env_build_amd.policy_grad import TrainableMLPNet

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=20); ap.add_argument('--windows', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_policy_grad_timing.txt'))
a = ap.parse_args()
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream()
med = lambda v: sorted(v)[len(v) // 2]
spread = lambda v: max(v) - min(v)
r = lambda v: round(v, 1)
lines = ['# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__)]
print(lines[0], flush=True)
p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters): fn()
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, iters):
    """{name: fn} -> {name: [us per call, one per window]}, the sides taking turns window by window"""
    for fn in fns.values():
        for _ in range(3): fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.windows):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def emit(what, times, iters, **extra):
    rec = dict(what=what, iters=iters, **extra)
    for k, v in times.items():
        rec[k + '_us'] = r(med(v)); rec[k + '_us_windows'] = [r(x) for x in v]; rec[k + '_spread_us'] = r(spread(v))
    rec['faster'] = min(times, key=lambda k: med(times[k]))
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def backward_case(what, n, obs_dim):
    rng = np.random.default_rng(0)
    net = TrainableMLPNet(obs_dim, 2, 256, 'elu', 4, device=dev)
    scale = rng.uniform(0.02, 0.2, obs_dim).astype(np.float32)
    net.set_obs_scale(scale)
    net._sync()
    obs = torch.from_numpy((rng.standard_normal((n, obs_dim)) * 10).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32)).to(dev)
    need = C.c_size_t(0)
    net.api.mlp_backward_workspace_bytes(net._h, n, C.byref(need))
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    out, g_obs, g_par = torch.empty((n, 4), device=dev), torch.empty_like(obs), torch.empty_like(net._flat)
    ours = lambda: net.api.mlp_backward(net._h, n, p(obs), p(g), 0, C.c_float(1.0), p(ws), need.value, p(out), p(g_obs), p(g_par), _stream(dev))
    # the twin: the same layers as torch.nn.Linear, the scale as a multiply, fp32
    w = net.get_weights()
    twin = torch.nn.Sequential(torch.nn.Linear(obs_dim, 256), torch.nn.ELU(), torch.nn.Linear(256, 256), torch.nn.ELU(), torch.nn.Linear(256, 4)).to(dev)
    with torch.no_grad():
        for lin, k, b in zip([twin[0], twin[2], twin[4]], w[0::2], w[1::2]):
            lin.weight.copy_(torch.from_numpy(k.T)); lin.bias.copy_(torch.from_numpy(b))
    sc = torch.from_numpy(scale).to(dev)
    x = obs.clone().requires_grad_(True)
    params = list(twin.parameters())

    def theirs():
        torch.autograd.grad(twin(x * sc), [x] + params, g)

    ours(); torch.cuda.synchronize()
    want = torch.autograd.grad(twin(x * sc), [x] + params, g)
    err = float((g_obs - want[0]).abs().max() / want[0].abs().max())
    emit(what, alternate({'eb_mlp_backward': ours, 'torch_twin_forward_backward': theirs}, a.iters), a.iters, n=n,
         net='%d -> 256 -> 256 -> 4, elu / linear, scale set; out, g_obs and g_params' % obs_dim, workspace_mb=r(need.value / 2 ** 20),
         g_obs_max_rel_diff_from_twin=err)
    return net


net = backward_case('backward', 65536, 137)
backward_case('small', 4096, 41)

# the weight update: device-side against the host path (which creates a new handle and synchronises)
host = MLPNet(137, 2, 256, 'elu', 4, device=dev)
weights = host.get_weights()
fns = {'eb_mlp_set_params_device': lambda: net.api.mlp_set_params_device(net._h, p(net._flat), _stream(dev)),
       'set_weights_through_the_host': lambda: host.set_weights(weights)}
emit('weights', alternate(fns, a.iters), a.iters, net='137 -> 256 -> 256 -> 4')
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')
