"""The table behind tests/test_stream_census.py and tests/test_gpu_capture.py: for every entry of include/*.h that takes a
`void* stream` parameter, either a row of CAPTURED — how to issue it on a stream of the caller's, and how many kernel nodes a capture of it must
hold — or a member of NOT_CAPTURED with the reason.  A helper module like _tape.py and _policy.py: pytest does not collect it, and
importing it touches no device (rows allocate when their `make` is called).

One spelling per call.  A row does not restate an entry's argument list: it runs the helper the existing tests use (DeviceModel.*,
TapeModel.t_*, the `entry` / `backward` functions of the policy tests) under `record`, which splits that helper into "allocate" and
"call": the helper allocates and stages as always, every C call it makes with the model's stream is NOTED instead of issued, and the
noted calls — the same function objects, the same argument objects — are what `Call.run(raw_stream)` issues, with nothing but the
stream replaced.  run() therefore makes no allocation, no host read and no synchronisation.

Which buffer is what follows from the header and from where the buffer came from: a device tensor is an INPUT when the helper staged
it from host data (DeviceModel._in: the in-place state of eb_env_step included) or when every recorded call takes it through a
`const` parameter; every other tensor a recorded call was given (also through a struct) is an OUTPUT.  Names are the header's
parameter names ('flow.timer', 'auto_reset.final_obs' for an array a struct argument points to)."""
import collections
import ctypes as C
import glob
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = {'A': 3, 'B': 4}
TASK, N_VEH, D = 'left', 8, 41
NET = (2, 64, 4)                                      # policy 41 -> 2 x 64 -> 4
K = 3                                                 # candidates / samples
W5 = (-1.0, 10.0, 0.0, 0.0, 0.0)
SAMPLE_SEED, SAMPLE_COUNTER = 0x1234567, 5


# ---- the headers ----
def stream_entries(include_dir=None):
    """every `int eb_*( ... void* stream ... );` of include/*.h, comments stripped -> {name: [(is_const_pointer, parameter name), ...]}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(include_dir or os.path.join(ROOT, 'include'), '*.h'))):
        with open(path) as fh:
            text = fh.read()
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        text = re.sub(r'//[^\n]*', ' ', text)
        for m in re.finditer(r'\bint\s+(eb_\w+)\s*\(([^;{}()]*)\)\s*;', text):
            params = [' '.join(p.split()) for p in m.group(2).split(',')]
            if not any(re.fullmatch(r'void\s*\*\s*stream', p) for p in params):
                continue
            assert m.group(1) not in out, '%s declared twice' % m.group(1)
            out[m.group(1)] = [(p.startswith('const ') and '*' in p, re.search(r'(\w+)$', p).group(1)) for p in params]
    return out


def _stripped(path):
    with open(path) as fh:
        text = fh.read()
    return re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))


def struct_stream_entries(include_dir=None):
    """every `int eb_*( ... const <struct>* ... );` of include/*.h whose argument struct carries a `void* stream` field, directly or in
    a member struct (eb_adam_ctl_args holds an eb_adam_args), comments stripped -> {name: the struct's name}.  The entries
    stream_entries() cannot see: the stream is no parameter of theirs."""
    paths = sorted(glob.glob(os.path.join(include_dir or os.path.join(ROOT, 'include'), '*.h')))
    texts = [_stripped(p) for p in paths]
    fields = {}
    for text in texts:
        for m in re.finditer(r'\btypedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', text):
            assert m.group(2) not in fields, '%s defined twice' % m.group(2)
            fields[m.group(2)] = [' '.join(f.split()) for f in m.group(1).split(';') if f.strip()]

    def has_stream(name, seen=()):
        for f in fields.get(name, ()):
            if re.fullmatch(r'void\s*\*\s*stream', f):
                return True
            member = re.fullmatch(r'(?:struct\s+)?(\w+)\s+\w+(?:\s*\[[^\]]*\])?', f)       # a struct held by value
            if member and member.group(1) in fields and member.group(1) not in seen and has_stream(member.group(1), seen + (name,)):
                return True
        return False
    out = {}
    for text in texts:
        for m in re.finditer(r'\bint\s+(eb_\w+)\s*\(([^;{}()]*)\)\s*;', text):
            for p in m.group(2).split(','):
                a = re.fullmatch(r'(?:const\s+)?(?:struct\s+)?(\w+)\s*\*\s*\w+', ' '.join(p.split()))
                if a and has_stream(a.group(1)):
                    assert m.group(1) not in out, '%s declared twice' % m.group(1)
                    out[m.group(1)] = a.group(1)
    return out


# entry -> (module of tests/, the test function that issues it on the null stream, on a side stream and under capture with replays).  An
# entry that joins the ABI with its stream inside a struct fails tests/test_stream_census.py until it has such a test and a row here.
STRUCT_STREAM_HELD = {
    'eb_policy_rollout_sample': ('test_gpu_policy_rollout_sample', 'test_side_stream_and_capture'),
    'eb_policy_logp': ('test_gpu_policy_logp', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_policy_logp_from_logits': ('test_gpu_policy_logp', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_policy_logp_vjp': ('test_gpu_policy_logp', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_ppo_surrogate': ('test_gpu_ppo', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_ppo_surrogate_from_logits': ('test_gpu_ppo', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_gae': ('test_gpu_ppo', 'test_side_stream_capture_and_replay_for_the_three_entries'),
    'eb_value_loss': ('test_gpu_train', 'test_both_entries_on_a_side_stream_and_under_capture'),
    'eb_adam_step': ('test_gpu_train', 'test_both_entries_on_a_side_stream_and_under_capture'),
    'eb_minibatch_gather': ('test_gpu_epoch', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_adv_stats': ('test_gpu_epoch', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_ppo_log': ('test_gpu_epoch', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_epoch_advance': ('test_gpu_epoch', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_collect_begin': ('test_gpu_collect', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_collect_record': ('test_gpu_collect', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_collect_next_values': ('test_gpu_collect', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_collect_episode_log': ('test_gpu_collect', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_ctl_begin': ('test_gpu_ctl', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_kl_stop': ('test_gpu_ctl', 'test_every_entry_on_a_side_stream_and_under_capture'),
    'eb_adam_step_ctl': ('test_gpu_ctl', 'test_every_entry_on_a_side_stream_and_under_capture'),
}


def function_text(module, name):
    """the source of tests/<module>.py's function `name` plus that of the module-level functions it calls by name (one level: the
    capture tests of two modules keep their raw calls in a `capture_cases()` of their own); None when there is no such function"""
    import ast
    with open(os.path.join(ROOT, 'tests', module + '.py')) as fh:
        src = fh.read()
    defs = {n.name: n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}
    if name not in defs:
        return None
    called = {c.func.id for c in ast.walk(defs[name]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
    return '\n'.join(ast.get_source_segment(src, defs[n]) for n in [name] + sorted(called & (set(defs) - {name})))


# ---- allocate | call ----
class Call(object):
    """inputs / outputs: name -> device tensor (allocated once; overwrite in place); initial: the inputs' contents as made;
    run(raw_stream): the C call(s), nothing else; dev: the model whose helper was recorded"""

    def __init__(self):
        self.inputs, self.outputs, self.initial, self.calls, self.keep, self.dev = {}, {}, {}, [], [], None

    def run(self, raw_stream):
        s = C.c_void_p(raw_stream)
        for fn, args in self.calls:
            fn(*args, s)


def record(dev, body, only=None):
    """body(dev) with every stream-taking C call noted, not issued -> Call.  only: the names (without eb_) to note; the other calls
    body makes are issued as usual, on the null stream (how a row prepares an input that an earlier call of the helper computes)."""
    entries = stream_entries()
    call, api, token, cls = Call(), dev.api, C.c_void_p(0), type(dev)
    seen, by_pointer, in_struct = collections.OrderedDict(), {}, {}
    call.keep.append(dev)
    call.dev = dev

    def pointer_fields(obj, prefix):
        for fname, ftype in obj._fields_:
            v = getattr(obj, fname)
            if isinstance(v, C.Structure):
                for item in pointer_fields(v, prefix + fname + '.'):
                    yield item
            elif ftype is C.c_void_p and v:
                yield prefix + fname, v

    def note(t, staged=False):
        base = t if t._base is None else t._base
        e = seen.setdefault(base.untyped_storage().data_ptr(), dict(t=base, staged=False, const=False, mut=False, name=None))
        e['staged'] = e['staged'] or staged
        return e

    def _in(a, dtype=np.float32):
        t = cls._in(dev, a, dtype)
        if t is not None:
            note(t, True)
        return t

    def _ptr(t):
        if t is None:
            return None
        p = C.c_void_p(t.data_ptr())
        by_pointer[id(p)] = note(t)
        call.keep.append((p, t))
        return p

    class Noting(object):
        def __getattr__(self, name):
            real = getattr(api, name)
            if not callable(real):
                return real

            def fn(*args):
                if not (args and args[-1] is token):
                    return real(*args)
                if only is not None and name not in only:
                    return real(*args[:-1], None)
                params = entries['eb_' + name]
                assert len(params) == len(args), 'eb_%s: %d arguments for %d parameters' % (name, len(args), len(params))
                for a, (is_const, pname) in zip(args[:-1], params):
                    if isinstance(getattr(a, '_obj', None), C.Structure):       # byref(struct): the arrays it points to, by field name
                        in_struct.update((addr, name) for name, addr in pointer_fields(a._obj, pname + '.'))
                    e = by_pointer.get(id(a))
                    if e is not None:
                        e['const' if is_const else 'mut'] = True
                        e['name'] = e['name'] or pname
                call.calls.append((real, args[:-1]))
            return fn

    stream = dev.stream
    dev.api, dev._in, dev._ptr, dev.stream = Noting(), _in, _ptr, token
    try:
        body(dev)
    finally:
        dev.api, dev.stream = api, stream
        del dev._in, dev._ptr
    assert call.calls, 'the helper made no stream-taking call'
    for e in seen.values():
        if not (e['const'] or e['mut']):
            if e['t'].data_ptr() not in in_struct:
                continue                             # staged or allocated by the helper, but given to no noted call
            e['mut'] = True                          # reached the call inside a struct (eb_respawn, eb_flow_rule, ...)
        first = e['name'] or in_struct[e['t'].data_ptr()]
        name, k = first, 1
        while name in call.inputs or name in call.outputs:
            k += 1
            name = '%s_%d' % (first, k)
        (call.inputs if e['staged'] or not e['mut'] else call.outputs)[name] = e['t']
    call.initial = {k: v.clone() for k, v in call.inputs.items()}
    return call


# ---- scenes (the generators of the existing tests) ----
def _model(**kw):
    from tests._tape import TapeModel
    return TapeModel(TASK, n_veh=N_VEH, **kw)


def _case(m, size, which):
    from tests._tape import synthetic_case
    return synthetic_case(m, TASK, size['n'], size.get('H', 1), SEEDS[which])


def _host_case(m, size, which):
    """synthetic_case as NumPy arrays, ref_idx within 0..2 (the tape family's tests feed an out-of-range index; the others do not)"""
    obs0, tape, ri, pid, _, _ = _case(m, size, which)
    m.torch.cuda.synchronize()
    return obs0.cpu().numpy(), tape.cpu().numpy(), np.clip(ri.cpu().numpy(), 0, 2).astype(np.int32), pid


def _rows(a, n, which):
    """n rows of `a`, another n for B (wrapping around when `a` is shorter)"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.resize(np.roll(a, -137 if which == 'B' else 0, axis=0), (n,) + a.shape[1:]))


def _policy_scene(size, which, f16=False):
    from tests._policy import f16_mlp, scene
    obs0, ref_idx, net, scale = scene(TASK, N_VEH, NET[1], NET[0], B=400)
    m = _model()
    mlp = f16_mlp(m, *net, scale) if f16 else m.make_mlp(*net, scale)
    return m, mlp, net, _rows(obs0, size['n'], which), _rows(ref_idx, size['n'], which).astype(np.int32)


def _env_scene(size, which, M=14, task=TASK):
    from env_build_amd import _capi
    from env_build_amd.endtoend_env_utils import VEHICLE_MODE_LIST
    from tests._env_step_check import random_scene
    from tests._tape import TapeModel
    B, seed = size['n'], 44 + SEEDS[which]
    native = VEHICLE_MODE_LIST[task]
    modes = [native[i % len(native)] for i in range(M)]
    ego, cand, _, lw, light, _, ref = random_scene(task, B, M, seed)
    cmode = np.tile(np.array([_capi.VMODE_ID[x] for x in modes], np.uint8), (B, 1))
    rng = np.random.default_rng(seed + 1)
    cmode[rng.random((B, M)) < 0.05] = _capi.VMODE_EMPTY
    s = dict(ego=ego, cand=cand, cmode=cmode, lw=lw, light=light, ref=ref, modes=modes,
             raw=rng.uniform(-1.2, 1.2, (B, 2)).astype(np.float32), virtual=(rng.random(B) < 0.3).astype(np.uint8),
             v_light=rng.integers(0, 4, B).astype(np.uint8), params=rng.normal(size=(B, 4)).astype(np.float32))
    s['entry'] = np.stack([rng.uniform(-60, 60, M), rng.uniform(-60, 60, M), rng.choice([0., 90., 180., -90.], M),
                           rng.choice([-1., 0., 1.], M), rng.choice([-1., 0., 1.], M)], 1).astype(np.float32)
    s['m'], s['tr'] = TapeModel(task, mode='training'), TapeModel(task, n_veh=M, modes=modes)
    s['obs0'] = s['m'].get_obs(ego, cand, cmode, light, ref_idx=ref)
    return s


# ---- rows: make(size, which) -> Call; which = 'A' or 'B' (the same shapes and scalars, other contents) ----
def _rollout_step(size, which, f16=False):
    m = _model()
    obs, tape, ri, pid = _host_case(m, size, which)
    if f16:
        u16 = obs.astype(np.float16).view(np.uint16)
        return record(m, lambda d: d.rollout_step_f16(u16, tape[0], ri, pid))
    return record(m, lambda d: d.rollout_step(obs, tape[0], ri, pid))


def _rollout_tape(size, which, f16=False):
    m = _model()
    obs, tape, ri, pid = _host_case(m, size, which)
    if f16:
        u16 = obs.astype(np.float16).view(np.uint16)
        return record(m, lambda d: d.rollout_tape_f16(u16, tape, ri, pid))
    return record(m, lambda d: d.rollout_tape(obs, tape, ri, pid))


def _rollout_acc(size, which):
    m = _model()
    obs, tape, ri, pid = _host_case(m, size, which)
    return record(m, lambda d: d.rollout_acc(obs, tape, ri, pid))


def _episode_summary(size, which):
    m = _model()
    obs, tape, ri, pid = _host_case(m, size, which)
    out, out5 = m.rollout_tape(obs, tape, ri, pid)
    return record(m, lambda d: d.episode_summary(out5, out))


def _small(method, args):
    """a row for one of the small single-kernel entries: DeviceModel.<method>(*args(obs, actions, ref_idx, path_id))"""
    def make(size, which):
        m = _model()
        obs, tape, ri, pid = _host_case(m, size, which)
        act = m.action_transform(tape[0])
        return record(m, lambda d: getattr(d, method)(*args(obs, act, ri, pid, tape[0])))
    return make


def _get_obs(size, which, task=TASK):
    s = _env_scene(size, which, task=task)
    return record(s['m'], lambda d: d.get_obs(s['ego'], s['cand'], s['cmode'], s['v_light'], ref_idx=s['ref'], virtual=s['virtual']))


def _env_step(size, which, task=TASK, auto_reset=False, time_limit=False):
    """auto_reset: with the pool's reset of the envs the step finishes (eb_auto_reset); time_limit: with eb_time_limit"""
    s = _env_scene(size, which, task=task)
    kw = {}
    if auto_reset:
        from env_build_amd.endtoend import _lane_entry
        entry = np.array([list(_lane_entry(x)[:3]) + list(_lane_entry(x)[3]) for x in s['modes']], np.float32)
        kw['auto_reset'] = dict(seed=99, counter=5, training=1, pool=dict(entry=entry, span=60.0, v_max=8.0, seed=4242, counter=17, edge_span=5.0))
    if time_limit:
        kw['time_limit'] = (np.random.default_rng(SEEDS[which]).integers(0, 205, size['n']).astype(np.int32), 200)
    c = record(s['m'], lambda d: d.env_step(s['tr'], s['obs0'], s['raw'], s['ego'], s['cand'], s['cmode'], ref_idx=s['ref'], cand_lw=s['lw'],
                                            v_light=s['v_light'], virtual=s['virtual'], **kw))
    c.keep.append(s['tr'])
    return c


def _flow_scene(size, which, K=2, task=TASK):
    """the scene of _env_step_check.flow_auto_reset_case: the flow source with a sixth of the egos off the road, so that a step
    finishes envs"""
    from env_build_amd import _capi
    from env_build_amd.synthetic import make_rollout_inputs
    from env_build_amd.traffic import ACCEL, EXIT_RANGE, FLOWS, LANE_START, ROUTES, VTYPES, approach_lane
    from tests._tape import TapeModel
    B, M, seed = size['n'], 12 * K, 13 + SEEDS[which]
    slot_modes = [r for r in ROUTES for _ in range(K)]
    lane = np.array([list(approach_lane(x)[0]) + list(approach_lane(x)[1]) for x in slot_modes], np.float32)
    period = (np.array([3600.0 / FLOWS[r][0] for r in ROUTES], np.float32) / 8).astype(np.float32)
    vmax = np.array([VTYPES[FLOWS[x][1]][2] for x in slot_modes], np.float32)
    clen = np.array([VTYPES[FLOWS[x][1]][0] for x in slot_modes], np.float32)
    lw = np.tile(np.array([[VTYPES[FLOWS[x][1]][0], VTYPES[FLOWS[x][1]][1]] for x in slot_modes], np.float32), (B, 1, 1))
    rng = np.random.default_rng(seed)
    inp = make_rollout_inputs(task, B, 8, 1, seed=seed)
    ego, ref = inp['ego'].copy(), inp['ref_idx'].copy()
    ego[::6, 3] += rng.uniform(7, 12, len(ego[::6])) * rng.choice([-1, 1], len(ego[::6]))
    m, tr = TapeModel(task, mode='training'), TapeModel(task, n_veh=M, modes=slot_modes)
    active = (rng.random((B, M)) < 0.4).astype(np.uint8)
    along = rng.uniform(0, 95, (B, M)).astype(np.float32)
    cand = np.stack([lane[None, :, 0] + along * lane[None, :, 3], lane[None, :, 1] + along * lane[None, :, 4],
                     rng.uniform(0, 9, (B, M)).astype(np.float32), np.broadcast_to(lane[None, :, 2], (B, M))], 2).astype(np.float32)
    mode = np.where(active != 0, np.array([_capi.VMODE_ID[x] for x in slot_modes], np.uint8)[None, :], _capi.VMODE_EMPTY).astype(np.uint8)
    timer = (rng.random((B, 12)) * period).astype(np.float32)
    emitted, sim_step = np.zeros((B, 12), np.int32), rng.integers(0, 600, B).astype(np.int32)
    light, virtual = rng.integers(0, 4, B).astype(np.uint8), (rng.random(B) < 0.3).astype(np.uint8)
    return dict(m=m, tr=tr, K=K, ego=ego, ref=ref, cand=cand, mode=mode, lw=lw, light=light, virtual=virtual, clen=clen,
                obs=m.get_obs(ego, cand, mode, light, ref_idx=ref, virtual=virtual), raw=rng.uniform(-1.0, 1.0, (B, 2)).astype(np.float32),
                mask=(rng.random(B) < 0.3).astype(np.uint8), phase0=np.full(B, 9, np.uint8), lane_len=LANE_START - 25.0,
                flow=dict(per_route=K, lane=lane, period=period, v_max=vmax, dt=0.1, exit_range=EXIT_RANGE, accel=ACCEL,
                          lane_len=LANE_START - 25.0, light_cycle=0, seed=99, active=active, timer=timer, emitted=emitted, sim_step=sim_step,
                          counter=1))


def _env_step_auto_reset_flow(size, which, task=TASK, auto_reset=True):
    """auto_reset False: the step with the flow rule alone"""
    s = _flow_scene(size, which, task=task)
    reset = dict(seed=777, counter=1, training=1, flow=dict(cand_len=s['clen'], phase0=s['phase0'], random_phase=0, seed=4242, counter=1))
    if not auto_reset:
        reset = None
    c = record(s['m'], lambda d: d.env_step(s['tr'], s['obs'], s['raw'], s['ego'], s['cand'], s['mode'], ref_idx=s['ref'], cand_lw=s['lw'],
                                            v_light=s['light'], virtual=s['virtual'], flow=s['flow'], auto_reset=reset))
    c.keep.append(s['tr'])
    return c


def _flow_step(size, which):
    s = _flow_scene(size, which)
    f = s['flow']
    return record(s['tr'], lambda d: d.traffic_flow_step(s['K'], s['cand'], f['active'], f['timer'], f['emitted'], f['sim_step'], f['lane'],
                                                         f['period'], f['v_max'], f['dt'], f['exit_range'], f['accel'], f['lane_len'], 1,
                                                         f['seed'], f['counter'], s['light']))


def _flow_reset(size, which):
    s = _flow_scene(size, which)
    f = s['flow']
    return record(s['tr'], lambda d: d.traffic_flow_reset(s['K'], s['mask'], s['ego'], s['cand'], f['active'], f['timer'], f['emitted'],
                                                          f['sim_step'], s['phase0'], f['lane'], f['period'], f['v_max'], s['clen'],
                                                          s['lane_len'], 0, 1, 4242, 1, s['mode'], s['light']))


def _env(method, args, handle='m'):
    """a row for one of the env-side single-kernel entries over _env_scene: <handle>.<method>(*args(scene))"""
    def make(size, which):
        s = _env_scene(size, which)
        c = record(s[handle], lambda d: getattr(d, method)(*args(s)))
        c.keep.append(s)
        return c
    return make


def _env_reset_pool(size, which, task=TASK, M=12):
    from env_build_amd.endtoend import _lane_entry
    s = _env_scene(size, which, M=M, task=task)
    entry = np.array([list(_lane_entry(x)[:3]) + list(_lane_entry(x)[3]) for x in s['modes']], np.float32)
    rng = np.random.default_rng(21 + SEEDS[which])
    mask = (rng.random(size['n']) < 0.3).astype(np.uint8)
    obs = rng.normal(size=(size['n'], s['m'].D)).astype(np.float32)
    pool = dict(entry=entry, span=60.0, v_max=8.0, seed=4242, counter=17, edge_span=5.0)
    c = record(s['m'], lambda d: d.env_reset_pool(s['tr'], 99, 5, 1, s['ego'], s['params'], s['ref'], s['virtual'], s['v_light'], s['cand'],
                                                  s['cmode'], obs, pool, mask=mask))
    c.keep.append(s['tr'])
    return c


def _mlp(method, f16):
    def make(size, which):
        m, mlp, net, obs, _ = _policy_scene(size, which, f16)
        if method == 'forward':
            return record(m, lambda d: d.mlp_forward(mlp, NET[2], obs))
        return record(m, lambda d: d.policy_run_batch(mlp, NET[2] // 2, obs, 1.0))
    return make


def _shield(size, which):
    m, mlp, net, obs, ri = _policy_scene(size, which)
    return record(m, lambda d: d.shield_is_safe(mlp, obs, ri, 0, steps=size['H']))


def _tape_family(entry):
    def make(size, which):
        from tests._tape import WEIGHTS, candidate_tapes
        m = _model()
        obs0, tape, ri, pid, g_final, g5 = _case(m, size, which)
        if entry == 'step_vjp':
            return record(m, lambda d: d.t_step_vjp(obs0, tape[0].contiguous(), ri, pid, g_final, g5[0].contiguous()))
        if entry == 'chain_vjp':
            return record(m, lambda d: d.t_composed(obs0, tape, ri, pid, g_final, g5), only=('rollout_chain_vjp',))
        if entry == 'tape_vjp':
            return record(m, lambda d: d.t_tape_vjp(obs0, tape, ri, pid, g_final, g5, WEIGHTS[3]))
        if entry in ('cand', 'cand_vjp'):
            tapes = candidate_tapes(m, tape, K, SEEDS[which])
            if entry == 'cand':
                return record(m, lambda d: d.t_cand(obs0, tapes, ri, 0, None, pid, False, WEIGHTS[0]))
            return record(m, lambda d: d.t_cand_vjp(obs0, tapes, ri, 0, None, pid, False, WEIGHTS[0]))
        if entry == 'sample':
            return record(m, lambda d: d.t_sample(obs0, tape, K, ri, pid, seed=SAMPLE_SEED, counter=SAMPLE_COUNTER))
        assert entry == 'ilqr'       # an iteration with a line search needs the gains of one before it (issued here, on the null stream)
        first = m.t_ilqr(obs0, tape, ri, pid)
        return record(m, lambda d: d.t_ilqr(obs0, first['u'], ri, pid, x_nom=first['x'], gains=first['gains'], alphas=(1.0, 0.5),
                                            w5=WEIGHTS[3]))
    return make


def _policy_rollout(size, which):
    from tests.test_gpu_policy_rollout import entry
    m, mlp, net, obs, ri = _policy_scene(size, which, f16=True)
    return record(m, lambda d: entry(d, mlp, obs, size['H'], ri))


def _policy_rollout_grad(size, which):
    from tests._policy_rollout_grad import entry
    m, mlp, net, obs, ri = _policy_scene(size, which)
    return record(m, lambda d: entry(d, mlp, obs, size['H'], W5, ri))


def _mlp_backward(g_params):
    def make(size, which):
        from tests.test_gpu_policy_grad import backward
        m, mlp, net, obs, _ = _policy_scene(size, which)
        g = np.random.default_rng(SEEDS[which]).standard_normal((size['n'], NET[2])).astype(np.float32)
        want = ('out', 'g_obs', 'g_params') if g_params else ('out', 'g_obs')
        return record(m, lambda d: backward(d, mlp, (D,) + NET, obs, g, want=want))
    return make


def _set_params_then_forward(size, which):
    from tests.test_gpu_policy_grad import flat_of
    m, mlp, net, obs, _ = _policy_scene(size, which)
    flat = flat_of(net[6]) * np.float32(1.0 if which == 'A' else 0.75)

    def body(d):
        d.api.mlp_set_params_device(mlp, d._ptr(d._in(flat)), d.stream)
        d.mlp_forward(mlp, NET[2], obs)
    return record(m, body)


def _policy_sample(entry):
    def make(size, which):
        from env_build_amd import policy_sample as ps
        from tests.test_gpu_policy_sample import logits_case
        n = size['n']
        m, mlp, net, obs, _ = _policy_scene(size, which)
        ps.bind(m.api)                               # (the prototypes of include/envbuild_policy_sample.h on the library's functions)
        logits, eps, g_a, g_lp = (_rows(a, n, which) for a in logits_case(NET[2]))
        full = lambda d, shape: d.torch.full(shape, float('nan'), device=d.dev)
        p = lambda d, t: d._ptr(t)

        def fused(d):
            d.api.policy_sample(mlp, n, p(d, d._in(obs)), p(d, d._in(eps)), None, SAMPLE_SEED, SAMPLE_COUNTER, 1.0, p(d, full(d, (n, 2))),
                                p(d, full(d, (n,))), p(d, full(d, (n, 4))), p(d, full(d, (n, 2))), d.stream)

        def from_logits(d):      # eps NULL: drawn from (seed, counter, row)
            d.api.policy_sample_from_logits(n, NET[2], p(d, d._in(logits)), None, None, SAMPLE_SEED, SAMPLE_COUNTER, 1.0, p(d, full(d, (n, 2))),
                                            p(d, full(d, (n,))), p(d, full(d, (n, 2))), d.stream)

        def vjp(d):
            d.api.policy_sample_vjp(n, NET[2], p(d, d._in(logits)), p(d, d._in(eps)), 0.5, p(d, d._in(g_a)), p(d, d._in(g_lp)),
                                    p(d, full(d, (n, 4))), d.stream)
        c = record(m, {'fused': fused, 'from_logits': from_logits, 'vjp': vjp}[entry])
        c.keep.append(mlp)
        return c
    return make


# ---- the table ----
Row = collections.namedtuple('Row', 'make sizes kernels other_nodes')
BATCHES = ({'n': 65}, {'n': 200})
HORIZONS = ({'n': 65, 'H': 1}, {'n': 200, 'H': 1}, {'n': 65, 'H': 5}, {'n': 200, 'H': 5})
# include/envbuild_mlp_grad.h: "workspace ... contents undefined before and after"; envbuild_policy_rollout_grad.h: "its contents afterwards
# are unspecified" — a buffer of this name is not compared between two runs (it still must not change while a call is captured)
UNSPECIFIED = ('workspace',)
MEASURED = None        # the header gives no number: the count must not depend on n_env, is printed, and DESIGN.md records it


def row(make, sizes=BATCHES, kernels=MEASURED, other_nodes=()):
    return Row(make, tuple(sizes), kernels, tuple(other_nodes))


def entries_of(key):
    """'eb_a+eb_b/variant' -> ('eb_a', 'eb_b')"""
    return tuple(key.split('/')[0].split('+'))


def expected_kernels(r, size, counts):
    """the kernel nodes row r must show at `size`; counts: row key -> what the rows measured so far showed at the same n"""
    k = r.kernels
    if isinstance(k, tuple):
        return k[0] + counts[k[1]]
    return k(size) if callable(k) else k


# A key is 'entry', 'entry/variant' or 'entry+entry' (one row that issues both).  No row passes an unaligned array: torch's allocator
# hands out 512-byte aligned blocks, so eb_env_step / eb_env_reset_pool / eb_get_obs take their one-launch paths.  Their fallback
# paths (csrc/eb_capi.hip "separate launches") are exercised by no row: those of eb_env_step and eb_env_reset_pool allocate scratch
# with hipMallocAsync (and copy rows with hipMemcpyAsync), which the header's capture bullet excludes.
CAPTURED = collections.OrderedDict([
    ('eb_rollout_step', row(_rollout_step)),
    ('eb_rollout_step_f16', row(lambda s, w: _rollout_step(s, w, True))),
    ('eb_rollout_tape', row(_rollout_tape, HORIZONS)),
    ('eb_rollout_tape_f16', row(lambda s, w: _rollout_tape(s, w, True), HORIZONS)),
    ('eb_rollout_step_acc+eb_episode_acc_finish', row(_rollout_acc, ({'n': 65, 'H': 3}, {'n': 200, 'H': 3}))),
    ('eb_episode_summary', row(_episode_summary, ({'n': 65, 'H': 3}, {'n': 200, 'H': 3}))),
    ('eb_compute_rewards', row(_small('compute_rewards', lambda obs, act, ri, pid, raw: (obs, act)))),
    ('eb_get_obs', row(_get_obs)),
    # include/envbuild.h: "the HIP library runs them as ONE launch" under the alignment conditions every row meets
    ('eb_env_step', row(_env_step, kernels=1)),
    ('eb_env_step/auto_reset_flow', row(_env_step_auto_reset_flow, kernels=1)),
    ('eb_env_reset_pool', row(_env_reset_pool, kernels=1)),
    ('eb_mlp_forward', row(_mlp('forward', False))),
    ('eb_mlp_forward/f16', row(_mlp('forward', True))),
    ('eb_policy_run_batch', row(_mlp('run_batch', False))),
    ('eb_policy_run_batch/f16', row(_mlp('run_batch', True))),
    ('eb_shield_is_safe', row(_shield, ({'n': 65, 'H': 3}, {'n': 200, 'H': 3}))),
    # include/envbuild_grad.h: "One launch"; "`horizon` launches"
    ('eb_rollout_step_vjp', row(_tape_family('step_vjp'), kernels=1)),
    ('eb_rollout_chain_vjp', row(_tape_family('chain_vjp'), ({'n': 65, 'H': 3}, {'n': 200, 'H': 3}), kernels=lambda size: size['H'])),
    ('eb_rollout_tape_vjp', row(_tape_family('tape_vjp'), HORIZONS, kernels=1)),
    # include/envbuild_cand.h, envbuild_cand_grad.h, envbuild_sample.h, envbuild_ilqr.h: "One launch"
    ('eb_rollout_tape_cand', row(_tape_family('cand'), HORIZONS, kernels=1)),
    ('eb_rollout_tape_cand_vjp', row(_tape_family('cand_vjp'), HORIZONS, kernels=1)),
    ('eb_rollout_tape_sample', row(_tape_family('sample'), HORIZONS, kernels=1)),
    ('eb_rollout_tape_ilqr', row(_tape_family('ilqr'), HORIZONS, kernels=1)),
    # include/envbuild_policy_rollout.h: "ALWAYS one launch"; envbuild_policy_rollout_grad.h: "ALWAYS the same three launches"
    ('eb_policy_rollout', row(_policy_rollout, ({'n': 65, 'H': 1}, {'n': 65, 'H': 5}), kernels=1)),
    ('eb_policy_rollout_grad', row(_policy_rollout_grad, ({'n': 65, 'H': 1}, {'n': 200, 'H': 5}), kernels=3)),
    # include/envbuild_mlp_grad.h: "A fixed number of launches on `stream`, independent of n"; with g_params the number is the one
    # include/envbuild_policy_rollout_grad.h gives for the call it replaces: "eb_mlp_backward (three launches, the policy's forward
    # recomputed)".  Without g_params the headers give none: measured
    ('eb_mlp_backward', row(_mlp_backward(True), ({'n': 1}, {'n': 65}, {'n': 2049}), kernels=3)),
    ('eb_mlp_backward/no_g_params', row(_mlp_backward(False), ({'n': 1}, {'n': 65}, {'n': 2049}))),
    # the pack ("on `stream`, in one launch, with no host copy") plus the forward
    ('eb_mlp_set_params_device+eb_mlp_forward', row(_set_params_then_forward, kernels=(1, 'eb_mlp_forward'))),
    # include/envbuild_policy_sample.h: "ALWAYS exactly one launch"; "an elementwise kernel"
    ('eb_policy_sample', row(_policy_sample('fused'), kernels=1)),
    ('eb_policy_sample_from_logits', row(_policy_sample('from_logits'), kernels=1)),
    ('eb_policy_sample_vjp', row(_policy_sample('vjp'), kernels=1)),
    # small single-kernel entries of envbuild.h
    ('eb_f_xu', row(_small('f_xu', lambda obs, act, ri, pid, raw: (obs[:, :6], act, 0.1)))),
    ('eb_action_transform', row(_small('action_transform', lambda obs, act, ri, pid, raw: (raw,)))),
    ('eb_compute_next_obses', row(_small('compute_next_obses', lambda obs, act, ri, pid, raw: (obs, act, ri, pid)))),
    ('eb_ego_predict', row(_small('ego_predict', lambda obs, act, ri, pid, raw: (obs[:, :6], act)))),
    ('eb_veh_predict', row(_small('veh_predict', lambda obs, act, ri, pid, raw: (obs[:, 9:],)))),
    ('eb_env_ego_step', row(_small('env_ego_step', lambda obs, act, ri, pid, raw: (obs[:, :6], act)))),
    ('eb_phi_diff', row(_small('phi_diff', lambda obs, act, ri, pid, raw: (obs[:, 5] * np.float32(3.0),)))),
    ('eb_find_closest_point', row(_small('find_closest_point', lambda obs, act, ri, pid, raw: (obs[:, 3], obs[:, 4], ri, pid)))),
    ('eb_path_points', row(_small('path_points', lambda obs, act, ri, pid, raw: ((np.abs(obs[:, 3]) * 40).astype(np.int32), 0, ri, pid)))),
    ('eb_tracking_error', row(_small('tracking_error', lambda obs, act, ri, pid, raw: (obs[:, 3], obs[:, 4], obs[:, 5], obs[:, 0], 0, ri, pid)))),
    ('eb_ss', row(_small('ss', lambda obs, act, ri, pid, raw: (obs, raw, ri, pid, 0.1)))),
    ('eb_exit_frame', row(_env('exit_frame', lambda s: ((np.arange(len(s['ego'])) * 7 // 3 % 4).astype(np.uint8), s['ego'])))),
    ('eb_judge_done', row(_env('judge_done', lambda s: (s['ego'], s['params'], s['obs0'], s['cand'], s['cmode'], s['lw'], s['v_light'])))),
    ('eb_ego_dynamics', row(_env('ego_dynamics', lambda s: (s['ego'], s['params'])))),
    ('eb_env_reset', row(_env('env_reset', lambda s: (len(s['ego']), 99, 5, 1, s['ego'], s['params'], s['ref'], s['virtual'])))),
    ('eb_traffic_respawn', row(_env('traffic_respawn', lambda s: (s['cand'], s['entry'], 30.0, 60.0, 8.0, 0x1234567, 9, None, s['ego'], 5.0),
                                    handle='tr'))),
    ('eb_traffic_flow_step', row(_flow_step)),
    ('eb_traffic_flow_reset', row(_flow_reset)),
])

NOT_CAPTURED = {
    'eb_rollout_gated': 'spins on flags another stream raises: a replay without its producer would hang',
    'eb_gate_feed': 'spins on the flags eb_rollout_gated raises, on a stream of its own: a replay without its consumer would hang',
    'eb_plan_launch': 'is itself a graph launch (eb_plan_create captured the rollout already)',
    'eb_event_record': 'records a timing event, no work: nothing to hold a replay to',
}
