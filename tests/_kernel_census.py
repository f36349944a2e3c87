"""The kernel census: which kernels libenvbuild_hip.so holds, and which launch reaches each instantiation of the rollout and closed-loop
families.  A helper module like _capture_cases.py: pytest does not collect it, and importing it touches no device.

`library_kernels(path)` reads the kernel names out of the library's gfx950 code object (every kernel has a `<mangled name>.kd` descriptor
symbol) and parses family and template arguments from the Itanium name — no demangler, no external tool.

`HELD` has one row per instantiation of the nine rollout families of csrc/eb_rollout.hip (rollout_fused_*, rollout_tape_*,
rollout_gated_*) and the three closed-loop families (policy_rollout_kernel, policy_rollout_grad_kernel, policy_rollout_sample_kernel),
141 rows.  A row is a `Case` — the entry and the arguments that reach the kernel, launched and held against the oracle by
tests/test_gpu_kernel_census.py — or `Unreachable(reason)`; `Faulted(reason)` is the third kind, for a row whose launch faulted and whose
cause is not found (no launch is made for it; none today).  `COUNTED` maps every other family to its instantiation count.  A new kernel or
instantiation anywhere in the library fails tests/test_kernel_census.py until someone extends HELD or updates COUNTED.

`ENV_HELD` does the same for the one-launch env kernels of csrc/eb_env_step_body.h: env_step_kernel<TASK, ET, OBS, AUTO, NW> (45) and
env_reset_pool_kernel<TASK, ET, NW> (15) — 3 tasks x 5 shapes (64-env tiles with four waves, 32- and 16-env tiles with four and eight)
x 4 kinds (step, step + auto reset, observation, masked reset), 60 rows, every one a Case, launched with the tile AND the waves per block
forced and held against the oracle by tests/test_gpu_env_census.py.  The four-wave kernels of the small tiles run in production only
above 3 * n_cu blocks; no test of the suite is that large on the small tiles, so before these rows nothing launched those 24 kernels.
`ENV_FEATURES` adds the rows that reach code only some calls switch on: the flow rule (on 16-env tiles x four waves: FUSED_FLOW), the
flow rule with auto reset (there: DRAW_LATE), and the episode step limit (its wave depends on NW).  `claimed_env_kernel(case)` restates
launch_env_step's rule.  The <RT, CT> policy kernels (mlp_f16_kernel, policy_sample_kernel, policy_logp_kernel, ppo_surrogate_kernel,
mlp_bwd_data_kernel) stay counted: their own modules run one width per instantiation.

The witness — which kernels a call enqueues — is read from the hipGraph a stream capture of the call produces (tests/_capture.py):
hipGraphKernelNodeGetParams gives each kernel node's host-side handle, `handle_names` maps the handles of the library's kernels (dynamic
symbols for the rollout families, local symbols of the unstripped library for the closed-loop ones, which live in an anonymous namespace)
to their mangled names.  `claimed_kernel(case)` restates the host's three launch rules (csrc/eb_rollout.hip: launch_rollout_fused,
launch_rollout_tape_fused, tape_tile_variant; the width switch of the closed-loop launchers) and is what ties a Case to its key; the
same rules with eb_debug_rollout_plan's (variant, rolling) are the fallback witness `plan_kernel`."""
import collections
import ctypes as C
import re
import struct

TASKS = ('left', 'straight', 'right')                       # template argument TASK = _capi.TASK_ID
FUSED = ('rollout_fused_4x8', 'rollout_fused_4x4', 'rollout_fused_1x4')
TAPE = ('rollout_tape_4x8', 'rollout_tape_4x4', 'rollout_tape_1x4')
GATED = ('rollout_gated_4x8', 'rollout_gated_4x4', 'rollout_gated_1x4')
POLICY = ('policy_rollout_kernel', 'policy_rollout_grad_kernel', 'policy_rollout_sample_kernel')
HELD_FAMILIES = FUSED + TAPE + GATED + POLICY
ENV_FAMILIES = ('env_step_kernel', 'env_reset_pool_kernel')
ALL_HELD_FAMILIES = HELD_FAMILIES + ENV_FAMILIES
RECORD_WAVES = (4, 4, 1)                                    # rw of tile shape 0 / 1 / 2 (4x8, 4x4, 1x4)
TILE_RECORDS = (4 * 64 * 8, 4 * 64 * 4, 1 * 64 * 4)         # fused_tile_records
WIDTH_OF = {(1, 1): 64, (2, 1): 128, (2, 2): 256}           # the closed-loop kernels' <RT, CT> per (padded) hidden-layer width
POLICY_ENTRY = {'policy_rollout_kernel': 'policy_rollout', 'policy_rollout_grad_kernel': 'policy_rollout_grad',
                'policy_rollout_sample_kernel': 'policy_rollout_sample'}

Kernel = collections.namedtuple('Kernel', 'family args symbol')     # args: tuple of int / bool / 'f32' / 'f16', None when not parsed
# (waves, auto_reset: the env rows' — eb_debug_set_env_waves 4 / 8, or 0 = by grid size; eb_env_step with / without eb_auto_reset)
Case = collections.namedtuple('Case', 'entry task n_veh tile rolling storage mode units waves auto_reset', defaults=(None, None))
Unreachable = collections.namedtuple('Unreachable', 'reason')
Faulted = collections.namedtuple('Faulted', 'reason')

_KD = re.compile(rb'(_Z[A-Za-z0-9_]+)\.kd\0')
_HEAD = re.compile(r'_ZN2eb(?:12_GLOBAL__N_1)?(\d+)')
_ARG = re.compile(r'Li(\d+)E|Lb([01])E|(DF16_)|(f)')


def parse(symbol):
    """mangled kernel name -> Kernel.  `_ZN2eb[12_GLOBAL__N_1]<len><family>[I<args>E]E...`; the arguments understood are Li<n>E (int),
    Lb<0|1>E (bool), f (float) and DF16_ (_Float16) — an argument list with anything else gives args None (family still known)."""
    m = _HEAD.match(symbol)
    if not m:
        raise ValueError('not a kernel of namespace eb: %s' % symbol)
    at = m.end() + int(m.group(1))
    family, rest = symbol[m.end():at], symbol[at:]
    if not rest.startswith('I'):
        return Kernel(family, (), symbol)
    args, at = [], 1
    while not rest.startswith('E', at):
        a = _ARG.match(rest, at)
        if not a:
            return Kernel(family, None, symbol)
        args.append(int(a.group(1)) if a.group(1) else bool(int(a.group(2))) if a.group(2) else 'f16' if a.group(3) else 'f32')
        at = a.end()
    return Kernel(family, tuple(args), symbol)


def kernel_symbols(data):
    """the distinct `<name>.kd` descriptor names in the bytes of a library"""
    return sorted({m.group(1).decode() for m in _KD.finditer(data)})


def library_kernels(lib_path):
    """-> [Kernel] of the library's code object, sorted by symbol"""
    with open(lib_path, 'rb') as fh:
        return [parse(s) for s in kernel_symbols(fh.read())]


def key_of(k):
    return (k.family,) + tuple(k.args)


# ---- the launch rules, restated ----
def tile_records(tile):
    return TILE_RECORDS[tile]


def envs_per_tile(tile, n_veh):
    return max(1, min(64, TILE_RECORDS[tile] // n_veh))


def fast(tile, n_veh):
    return (RECORD_WAVES[tile] * 64) % n_veh == 0


def rollout_kernel(kind, task, n_veh, variant, rolling, storage):
    """the key of the kernel launch_rollout_fused ('fused') / launch_rollout_tape_fused ('tape', 'gated') launches for a tile shape that
    is already decided: rw from the variant, FAST = (rw * 64) % n_veh == 0, PF = 3 iff variant 0 and rolling (else 8 on the 4x8 tile, 4 on
    the others); an open-loop tape on the 4x8 tile whose slot count does not divide 256 lanes goes to the 4x4 tile (tape_tile_variant)"""
    t = TASKS.index(task)
    if kind == 'tape' and variant == 0 and (4 * 64) % n_veh != 0:
        variant = 1
    f = fast(variant, n_veh)
    if kind == 'fused':
        pf = 3 if (variant == 0 and rolling) else 8 if variant == 0 else 4
        return (FUSED[variant], t, f, pf, storage)
    return ((TAPE if kind == 'tape' else GATED)[variant], t, f, storage)


KIND_OF_ENTRY = {'rollout_step': 'fused', 'rollout_step_f16': 'fused', 'rollout_tape': 'tape', 'rollout_tape_f16': 'tape',
                 'rollout_gated': 'gated'}


def claimed_kernel(case):
    """the key of the kernel a Case says it launches (tile and schedule forced, as the GPU test forces them)"""
    if case.entry in KIND_OF_ENTRY:
        assert case.tile in (0, 1, 2) and case.rolling in (0, 1)
        return rollout_kernel(KIND_OF_ENTRY[case.entry], case.task, case.n_veh, case.tile, case.rolling, case.storage)
    family = {v: k for k, v in POLICY_ENTRY.items()}[case.entry]
    rt_ct = {v: k for k, v in WIDTH_OF.items()}[case.units]
    return (family, TASKS.index(case.task)) + rt_ct


def plan_kernel(case, plan):
    """the fallback witness: the key from eb_debug_rollout_plan's (variant, workgroups, rolling, by_progress) for the case's batch"""
    return rollout_kernel(KIND_OF_ENTRY[case.entry], case.task, case.n_veh, plan[0], plan[2], case.storage)


def batch_of(case):
    """two full tiles plus three envs: a second block and a ragged tail (closed-loop rows: one 64-row tile and one row)"""
    if case.entry in POLICY_ENTRY.values():
        return 65
    tile = case.tile
    if KIND_OF_ENTRY[case.entry] == 'tape' and tile == 0 and (4 * 64) % case.n_veh != 0:
        tile = 1
    return 2 * envs_per_tile(tile, case.n_veh) + 3


def scene_inputs(case, steps=3):
    """the seeded scene of a fused / tape / gated row: make_rollout_inputs at the row's batch (one scene per task, slot count and batch)"""
    from env_build_amd.synthetic import make_rollout_inputs
    B = batch_of(case)
    return make_rollout_inputs(case.task, B, case.n_veh, steps, seed=500 + 7 * TASKS.index(case.task) + case.n_veh + B)


# ---- the table ----
NATIVE = {'left': 8, 'straight': 9, 'right': 5}             # VEH_NUM
GATED_F16 = ('eb_rollout_gated is the only entry that launches rollout_gated_* and it never sets storage_f16 (RolloutLaunch::storage_f16 '
             'stays 0 and no include header declares a binary16 gated entry): compiled, resources queried by tape_blocks_per_cu, '
             'launched by nothing')


def slots(task, is_fast):
    """FAST rows use 16 slots (divides 64 and 256 lanes); not-FAST rows 9, or 5 on `right` — each task tiled in place"""
    return 16 if is_fast else 5 if task == 'right' else 9


def _held():
    rows = collections.OrderedDict()
    for tile, family in enumerate(FUSED):
        for t, task in enumerate(TASKS):
            for f in (False, True):
                for pf in ((3, 8) if tile == 0 else (4,)):
                    for st in ('f32', 'f16'):
                        rows[(family, t, f, pf, st)] = Case('rollout_step' if st == 'f32' else 'rollout_step_f16', task, slots(task, f),
                                                            tile, int(pf == 3), st, 'training', None)
    for tile, family in enumerate(TAPE):
        for t, task in enumerate(TASKS):
            for f in ((True,) if tile == 0 else (False, True)):          # the 4x8 tape tile exists FAST-only
                for st in ('f32', 'f16'):
                    rows[(family, t, f, st)] = Case('rollout_tape' if st == 'f32' else 'rollout_tape_f16', task, slots(task, f), tile, 0,
                                                    st, 'training', None)
    for tile, family in enumerate(GATED):
        for t, task in enumerate(TASKS):
            for f in (False, True):
                rows[(family, t, f, 'f32')] = Case('rollout_gated', task, slots(task, f), tile, 0, 'f32', 'training', None)
                rows[(family, t, f, 'f16')] = Unreachable(GATED_F16)
    for family in POLICY:
        for t, task in enumerate(TASKS):
            for rt_ct, units in sorted(WIDTH_OF.items()):
                rows[(family, t) + rt_ct] = Case(POLICY_ENTRY[family], task, NATIVE[task], None, None, 'f32', 'training', units)
    return rows


HELD = _held()

COUNTED = {
    'acc_fold_kernel': 1, 'action_transform_kernel': 1, 'copy_rows_masked_kernel': 1, 'ego_dynamics_kernel': 1, 'ego_predict_kernel': 1,
    'env_ego_step_kernel': 1, 'env_pre_kernel': 3, 'env_reset_kernel': 1, 'exit_frame_kernel': 1, 'f_xu_kernel': 1, 'flag_swap_kernel': 1, 'gae_kernel': 1, 'gate_feed_kernel': 1, 'get_obs_exit_kernel': 3,
    'get_obs_kernel': 6, 'judge_done_kernel': 1, 'mlp_bwd_data_kernel': 3, 'mlp_f16_kernel': 4, 'mlp_kernel': 4, 'mlp_pack_kernel': 1,
    'mlp_wgrad_kernel': 1, 'mlp_wgrad_reduce_kernel': 1, 'path_points_kernel': 1, 'phi_diff_kernel': 1, 'policy_logp_kernel': 4,
    'policy_logp_logits_kernel': 1, 'policy_logp_vjp_kernel': 1, 'policy_sample_kernel': 4, 'policy_sample_logits_kernel': 1,
    'policy_sample_vjp_kernel': 1, 'ppo_surrogate_kernel': 4, 'ppo_surrogate_logits_kernel': 1, 'rewards_kernel': 3,
    'rollout_step_vjp_kernel': 3, 'rollout_tape_cand_kernel': 6, 'rollout_tape_cand_vjp_kernel': 6, 'rollout_tape_ilqr_kernel': 3,
    'rollout_tape_sample_kernel': 3, 'rollout_tape_vjp_kernel': 12, 'ss_kernel': 3, 'summary_final_kernel': 1,
    'summary_partial_kernel': 1, 'time_limit_kernel': 1, 'tracking_kernel': 3, 'traffic_flow_reset_kernel': 1,
    'traffic_flow_step_kernel': 1, 'traffic_respawn_kernel': 1, 'veh_predict_kernel': 1,
}


# ---- the one-launch env kernels (csrc/eb_env_step.hip: launch_env_step; csrc/eb_env_step_body.h: launch_env_step_task) ----
ENV_SHAPES = ((64, 4), (32, 4), (32, 8), (16, 4), (16, 8))  # (ET, NW): eight waves per block exist for the 16- and 32-env tiles only
ENV_KINDS = ('step', 'auto', 'obs', 'reset')                # eb_env_step, eb_env_step + eb_auto_reset, eb_get_obs, eb_env_reset_pool
ENV_ENTRY = {'step': 'env_step', 'auto': 'env_step', 'obs': 'get_obs', 'reset': 'env_reset_pool'}
TILE_OF_ET = {64: 0, 32: 1, 16: 2}                          # eb_debug_set_tile on the env-side kernels
ENV_CAND = 14                                               # candidates per env of the pool rows (the flow rows: 12 K = 24)
FLOW_K = 2


def env_kind(case):
    return {'get_obs': 'obs', 'env_reset_pool': 'reset'}.get(case.entry) or ('auto' if case.auto_reset else 'step')


def env_key(kind, t, et, nw):
    if kind == 'reset':
        return ('env_reset_pool_kernel', t, et, nw)
    return ('env_step_kernel', t, et, kind == 'obs', kind == 'auto', nw)


def claimed_env_kernel(case, n_env=None, n_cu=None):
    """the key of the kernel an env Case says it launches: the kind from the entry and its arguments, ET from the forced tile, NW from
    the forced waves (eight exist below 64-env tiles only) or — waves 0 — from the grid: eight while n_blocks <= 3 * n_cu.  (A forced
    tile that does not fit the LDS falls back to 16-env tiles; the rows are shaped to fit and the GPU witness is the judge.)"""
    assert case.entry in ENV_ENTRY.values() and case.tile in (0, 1, 2) and case.waves in (0, 4, 8)
    et = {v: k for k, v in TILE_OF_ET.items()}[case.tile]
    if case.waves:
        eight = case.waves == 8
    else:
        eight = (n_env + et - 1) // et <= 3 * n_cu
    return env_key(env_kind(case), TASKS.index(case.task), et, 8 if eight and et <= 32 else 4)


def env_batch_of(case):
    """two full tiles plus three envs"""
    return 2 * {v: k for k, v in TILE_OF_ET.items()}[case.tile] + 3


def _env_held():
    rows = collections.OrderedDict()
    for kind in ENV_KINDS:
        for t, task in enumerate(TASKS):
            for et, nw in ENV_SHAPES:
                rows[env_key(kind, t, et, nw)] = Case(ENV_ENTRY[kind], task, NATIVE[task], TILE_OF_ET[et], None, 'f32', 'training', None,
                                                      nw, kind == 'auto')
    return rows


ENV_HELD = _env_held()
# the 24 kernels no test launched before these rows: the small tiles with four waves per block
ENV_NEW = [key for key in ENV_HELD if key[-1] == 4 and key[2] in (16, 32)]
# feature rows: (feature, key of the kernel the row runs on) — the flow rule on the 15 plain-step kernels, the flow rule with auto reset
# and the episode step limit on the 15 auto-reset kernels
ENV_FEATURES = ([('flow', k) for k in ENV_HELD if k[0] == 'env_step_kernel' and not k[3] and not k[4]] +
                [('flow_auto', k) for k in ENV_HELD if k[0] == 'env_step_kernel' and k[4]] +
                [('time_limit', k) for k in ENV_HELD if k[0] == 'env_step_kernel' and k[4]])
# what each row's scene is drawn with, per batch size (2 ET + 3) where it has to differ: seeds, close_p, steps and K are chosen so that the
# ORACLE meets the conditions of tests/test_env_census_scenes.py (a flow row emits and lets exit, an auto-reset row finishes envs in
# its first tile and outside it, a masked reset masks an env of the ragged tail) — conditions on the inputs, decided on the CPU
ENV_PARAMS = {                                              # None: every (task, B) of the kind; (task, B): that scene's own
    'step': {},
    'auto': {None: dict(seed=5, close_p=0.02)},
    'obs': {},
    'reset': {None: dict(seed=21), ('left', 67): dict(seed=23), ('straight', 35): dict(seed=22), ('right', 67): dict(seed=24)},
    'flow': {None: dict(steps=6, seed=3)},
    'flow_auto': {None: dict(steps=2, seed=13), ('right', 67): dict(seed=15)},
    'time_limit': {None: dict(seed=8)},
}


def env_params(kind, task, B):
    p = ENV_PARAMS[kind]
    return dict(p.get(None, {}), **p.get((task, B), {}))


def env_rows():
    """[(row id, kind or feature, key, Case)]: the 60 rows of ENV_HELD, then the 45 feature rows"""
    rows = [(row_id(k), env_kind(c), k, c) for k, c in ENV_HELD.items()]
    return rows + [('%s-%s' % (f, row_id(k)), f, k, ENV_HELD[k]) for f, k in ENV_FEATURES]


def census(kernels):
    """-> (held kernels that are no key of HELD / ENV_HELD, keys of the two the library lacks, {family: (found, expected)} where COUNTED
    disagrees), all empty when every kernel is accounted for"""
    rows = set(HELD) | set(ENV_HELD)
    held = {key_of(k): k for k in kernels if k.family in ALL_HELD_FAMILIES and k.args is not None}
    extra = sorted(k.symbol for key, k in held.items() if key not in rows)
    extra += sorted(k.symbol for k in kernels if k.family in ALL_HELD_FAMILIES and k.args is None)
    missing = sorted((key for key in rows if key not in held), key=row_id)
    found = collections.Counter(k.family for k in kernels if k.family not in ALL_HELD_FAMILIES)
    counts = {f: (found.get(f, 0), COUNTED.get(f, 0)) for f in set(found) | set(COUNTED) if found.get(f, 0) != COUNTED.get(f, 0)}
    return extra, missing, counts


def reachable():
    return [(key, row) for key, row in HELD.items() if isinstance(row, Case)]


def row_id(key):
    return '-'.join(str(int(a)) if isinstance(a, bool) else str(a) for a in key)


# ---- the witness comparison ----
def check_witness(key, launched):
    """`launched`: the keys of the kernels a row's call enqueued (held families only).  The row's kernel must be among them and no other
    kernel of the held families may be; AssertionError names both otherwise."""
    launched = set(launched)
    assert key in launched, 'the row claims %s, its call launches %s' % (row_id(key), sorted(row_id(k) for k in launched) or 'no held kernel')
    assert launched == {key}, 'the row claims %s, its call also launches %s' % (row_id(key), sorted(row_id(k) for k in launched - {key}))


def is_hip_error(e):
    """a HIP error (the card may have faulted: no more launches) as opposed to a failing comparison or a refused argument"""
    from env_build_amd import _capi
    if isinstance(e, AssertionError):
        return False
    text = str(e)                # an EbError from EB_HIP names the runtime call that failed (hipGetLastError(): ...); torch says 'HIP error'
    return (isinstance(e, _capi.EbError) and re.search(r'\bhip[A-Z]', text) is not None) or 'HIP error' in text or 'hipError' in text


# ---- host-side kernel handles of the loaded library ----
def elf_symbols(data):
    """{name: st_value} of the OBJECT symbols in an ELF64 little-endian file's .symtab (local symbols included)"""
    assert data[:6] == b'\x7fELF\x02\x01', 'not a 64-bit little-endian ELF file'
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for name, kind, flags, addr, off, size, link, info, align, entsize in sections:
        if kind != 2:                                       # SHT_SYMTAB
            continue
        str_off = sections[link][4]
        for at in range(off, off + size, entsize or 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from('<IBBHQQ', data, at)
            if st_info & 0xF == 1 and st_shndx:             # STT_OBJECT, defined
                end = data.index(b'\0', str_off + st_name)
                out[data[str_off + st_name:end].decode()] = st_value
    return out


def handle_names(lib_path, loaded):
    """{address in this process: Kernel} for the host-side handle of every kernel of the library: the OBJECT symbol that carries the
    kernel's mangled name.  `loaded`: the ctypes CDLL of the same file; the load base comes from a dynamic symbol's address"""
    with open(lib_path, 'rb') as fh:
        data = fh.read()
    table = elf_symbols(data)
    anchor = next(s for s in kernel_symbols(data) if s in table and parse(s).family in FUSED)      # (a dynamic symbol)
    base = C.addressof(C.c_char.in_dll(loaded, anchor)) - table[anchor]
    return {base + table[s]: parse(s) for s in kernel_symbols(data) if s in table}


class _Dim3(C.Structure):
    _fields_ = [('x', C.c_uint), ('y', C.c_uint), ('z', C.c_uint)]


class KernelNodeParams(C.Structure):                        # hipKernelNodeParams (hip_runtime_api.h)
    _fields_ = [('blockDim', _Dim3), ('extra', C.c_void_p), ('func', C.c_void_p), ('gridDim', _Dim3), ('kernelParams', C.c_void_p),
                ('sharedMemBytes', C.c_uint)]


def kernel_node_funcs(captured):
    """the `func` of every kernel node of a tests/_capture.Captured graph, in the graph's node order"""
    from tests import _capture
    hip = _capture.hip_runtime()
    hip.hipGraphKernelNodeGetParams.restype = C.c_int
    hip.hipGraphKernelNodeGetParams.argtypes = [C.c_void_p, C.POINTER(KernelNodeParams)]
    funcs = []
    for node in captured._nodes():
        kind = C.c_int(-1)
        _capture._check(hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)), '%s: hipGraphNodeGetType' % captured.what)
        if kind.value != 0:
            continue
        p = KernelNodeParams()
        _capture._check(hip.hipGraphKernelNodeGetParams(C.c_void_p(node), C.byref(p)), '%s: hipGraphKernelNodeGetParams' % captured.what)
        funcs.append(p.func)
    return funcs
