"""Builds env_build_amd/lib/libenvbuild_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

-ffp-contract=off is part of the numerical contract: every fp32 op of the reference is one IEEE
rounding, so no FMA contraction.

Staleness is decided by CONTENT, not by mtime: the SHA-256 of every source, header and compiler flag is
written next to the library (libenvbuild_hip.so.srchash) when it is built, and `needs_build()` /
`check_fresh()` compare it with the hash of the sources present.  A library that was copied somewhere
together with different sources (e.g. a snapshot pushed to a GPU box) is therefore never silently reused:
it is rebuilt when hipcc is there, and `_capi.hip_api()` refuses to load it otherwise.

`build_train()` does the same for env_build_amd/lib/libenvbuild_train.so, the training-only kernels (csrc/eb_train.hip): a library of its
own with its own source list and hash, which `env_build_amd.train` loads on first use and nothing else does.
`build_epoch()` likewise for env_build_amd/lib/libenvbuild_epoch.so (csrc/eb_epoch.hip), which `env_build_amd.epoch` loads, and
`build_collect()` for env_build_amd/lib/libenvbuild_collect.so (csrc/eb_collect.hip), which `env_build_amd.collect` loads, and
`build_ctl()` for env_build_amd/lib/libenvbuild_ctl.so (csrc/eb_ctl.hip), which `env_build_amd.ctl` loads, and
`build_ac()` for env_build_amd/lib/libenvbuild_ac.so (csrc/eb_ac.hip), which `env_build_amd.ac` loads, and
`build_norm()` for env_build_amd/lib/libenvbuild_norm.so (csrc/eb_norm.hip), which `env_build_amd.norm` loads, and
`build_offpolicy()` for env_build_amd/lib/libenvbuild_offpolicy.so (csrc/eb_offpolicy.hip), which `env_build_amd.offpolicy` loads, and
`build_per()` for env_build_amd/lib/libenvbuild_per.so (csrc/eb_per.hip), which `env_build_amd.per` loads."""
import hashlib
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'lib', 'libenvbuild_hip.so')
HASH_FILE = LIB + '.srchash'
SOURCES = ['eb_capi.hip', 'eb_kernels.hip', 'eb_rollout.hip', 'eb_env_kernels.hip', 'eb_env_step.hip', 'eb_env_step_t1.hip', 'eb_env_step_t2.hip',
           'eb_policy.hip', 'eb_rollout_vjp.hip', 'eb_rollout_tape_vjp.hip', 'eb_rollout_tape_cand.hip', 'eb_rollout_tape_cand_vjp.hip', 'eb_rollout_tape_sample.hip', 'eb_rollout_tape_ilqr.hip', 'eb_policy_f16.hip', 'eb_policy_rollout.hip', 'eb_policy_grad.hip', 'eb_policy_rollout_grad.hip', 'eb_policy_sample.hip', 'eb_policy_rollout_sample.hip', 'eb_policy_logp.hip', 'eb_ppo.hip']   # (the env step's kernels: one translation unit per task — the three compile side by side)
HEADERS = ['eb_device.h', 'eb_kernels.h', 'eb_mlp_device.h', 'eb_env_device.h', 'eb_env_step_body.h', os.path.join('..', '..', 'include', 'envbuild.h'),
           'eb_grad.h', 'eb_grad_device.h', 'eb_tape_grad_device.h', 'eb_tape_device.h', os.path.join('..', '..', 'include', 'envbuild_grad.h'),
           'eb_cand.h', os.path.join('..', '..', 'include', 'envbuild_cand.h'),
           'eb_cand_grad.h', os.path.join('..', '..', 'include', 'envbuild_cand_grad.h'),
           'eb_sample.h', os.path.join('..', '..', 'include', 'envbuild_sample.h'),
           'eb_ilqr.h', 'eb_ilqr_device.h', os.path.join('..', '..', 'include', 'envbuild_ilqr.h'),
           'eb_policy_f16.h', os.path.join('..', '..', 'include', 'envbuild_mlp_f16.h'),
           'eb_policy_f16_device.h', 'eb_policy_rollout.h', os.path.join('..', '..', 'include', 'envbuild_policy_rollout.h'),
           'eb_policy_grad.h', os.path.join('..', '..', 'include', 'envbuild_mlp_grad.h'),
           'eb_policy_rollout_grad.h',
           os.path.join('..', '..', 'include', 'envbuild_policy_rollout_grad.h'),
           'eb_policy_sample.h', 'eb_policy_sample_device.h', os.path.join('..', '..', 'include', 'envbuild_policy_sample.h'),
           'eb_policy_rollout_sample.h', os.path.join('..', '..', 'include', 'envbuild_policy_rollout_sample.h'),
           'eb_policy_head_device.h', 'eb_policy_logp.h', 'eb_policy_logp_device.h', os.path.join('..', '..', 'include', 'envbuild_policy_logp.h'),
           'eb_ppo.h', 'eb_ppo_device.h', os.path.join('..', '..', 'include', 'envbuild_ppo.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-fast-math',
         '-fPIC', '-Wno-unused-value', '-Wno-pass-failed',
         '-mllvm', '-amdgpu-kernarg-preload-count=14']   # the rollout kernel's leading arguments (14 dwords: all of FusedHot) arrive in SGPRs
LINK_FLAGS = ['--offload-arch=gfx950', '-shared', '-fPIC']


def source_hash():
    """SHA-256 over the compiler flags and the bytes of every source and header, in a fixed order."""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in SOURCES + HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


KERNEL_SOURCES = {   # what a kernel's machine code depends on (its translation unit and the headers it includes) — pmc_traffic.py
    'rollout': ['eb_rollout.hip', 'eb_device.h', 'eb_kernels.h'],             # records these next to the HBM bytes it measures,
    'env_step': ['eb_env_step_body.h', 'eb_env_step.hip', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h'],   # bench.py refuses the bytes of other code
}


def kernel_hash(which):
    """SHA-256 over the compiler flags and the sources of one kernel family ('rollout' / 'env_step')."""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS).encode())
    for f in KERNEL_SOURCES[which]:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def built_hash():
    try:
        with open(HASH_FILE) as fh:
            return fh.read().strip()
    except OSError:
        return None


def needs_build():
    return not os.path.isfile(LIB) or built_hash() != source_hash()


def check_fresh():
    """(ok, message): does the library on disk come from the sources on disk?"""
    if not os.path.isfile(LIB):
        return False, 'HIP extension missing: %s' % LIB
    if built_hash() != source_hash():
        return False, ('%s was built from different sources or flags than the ones in %s (hash %s, sources %s)'
                       % (LIB, CSRC, built_hash(), source_hash()))
    return True, ''


def build(force=False, verbose=False):
    """Compile the translation units in parallel (one hipcc per .hip file: a fresh GPU box builds the library in the time
    of its slowest file), then link; the library and its source hash are replaced atomically at the end."""
    if not force and not needs_build():
        return LIB
    import fcntl
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    # one builder at a time: the ranks of a multi-GPU job on a fresh box all arrive here; the first one compiles, the
    # others wait for the lock and find the library fresh
    with open(LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not needs_build():
            return LIB
        return _build_locked(verbose)


def _build_locked(verbose, lib=None, sources=None, digest=None):
    import shutil
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    lib, sources = lib or LIB, sources or SOURCES
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    digest = digest or source_hash()           # of what the compiler is about to read
    objdir = tempfile.mkdtemp(prefix='eb_build_', dir=os.path.dirname(lib))
    try:
        def compile_one(f):
            obj = os.path.join(objdir, os.path.splitext(f)[0] + '.o')
            cmd = [hipcc] + FLAGS + ['-c', os.path.join(CSRC, f), '-o', obj]
            if verbose:
                print(' '.join(cmd))
            subprocess.check_call(cmd)
            return obj
        with ThreadPoolExecutor(max_workers=min(len(sources), os.cpu_count() or 1)) as pool:
            objs = list(pool.map(compile_one, sources))
        tmp = lib + '.tmp%d' % os.getpid()
        cmd = [hipcc] + LINK_FLAGS + objs + ['-o', tmp]
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)
        os.replace(tmp, lib)
    finally:
        shutil.rmtree(objdir, ignore_errors=True)
    with open(lib + '.srchash', 'w') as fh:
        fh.write(digest + '\n')
    return lib


# ---- libenvbuild_train.so: the training-only kernels (include/envbuild_train.h).  A library of its own — libenvbuild_hip.so, SOURCES,
# HEADERS and source_hash() know nothing of it — built with the same flags, the same content-hash staleness rule, the same lock
# discipline and the same atomic replace. ----
TRAIN_LIB = os.path.join(HERE, 'lib', 'libenvbuild_train.so')
TRAIN_SOURCES = ['eb_train.hip']
TRAIN_HEADERS = ['eb_train.h', 'eb_train_device.h', os.path.join('..', '..', 'include', 'envbuild_train.h'),
                 os.path.join('..', '..', 'include', 'envbuild.h')]


def train_source_hash():
    """source_hash() of the training library: the flags and the bytes of TRAIN_SOURCES and TRAIN_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in TRAIN_SOURCES + TRAIN_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def train_needs_build():
    try:
        with open(TRAIN_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(TRAIN_LIB) or built != train_source_hash()


def build_train(force=False, verbose=False):
    """build() for libenvbuild_train.so"""
    if not force and not train_needs_build():
        return TRAIN_LIB
    import fcntl
    os.makedirs(os.path.dirname(TRAIN_LIB), exist_ok=True)
    with open(TRAIN_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not train_needs_build():
            return TRAIN_LIB
        return _build_locked(verbose, TRAIN_LIB, TRAIN_SOURCES, train_source_hash())


# ---- libenvbuild_epoch.so: the kernels around the minibatch chain — keyed gather, advantage statistics, logging sums, the iteration
# counter (include/envbuild_epoch.h).  A third library of its own, built the way the second one is.  eb_epoch_device.h takes splitmix64
# from eb_env_device.h, so that header and what it includes are part of this library's hash too (and stay in HEADERS, unchanged). ----
EPOCH_LIB = os.path.join(HERE, 'lib', 'libenvbuild_epoch.so')
EPOCH_SOURCES = ['eb_epoch.hip']
EPOCH_HEADERS = ['eb_epoch.h', 'eb_epoch_device.h', os.path.join('..', '..', 'include', 'envbuild_epoch.h'),
                 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h', os.path.join('..', '..', 'include', 'envbuild.h')]


def epoch_source_hash():
    """source_hash() of the epoch library: the flags and the bytes of EPOCH_SOURCES and EPOCH_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in EPOCH_SOURCES + EPOCH_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def epoch_needs_build():
    try:
        with open(EPOCH_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(EPOCH_LIB) or built != epoch_source_hash()


def build_epoch(force=False, verbose=False):
    """build() for libenvbuild_epoch.so"""
    if not force and not epoch_needs_build():
        return EPOCH_LIB
    import fcntl
    os.makedirs(os.path.dirname(EPOCH_LIB), exist_ok=True)
    with open(EPOCH_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not epoch_needs_build():
            return EPOCH_LIB
        return _build_locked(verbose, EPOCH_LIB, EPOCH_SOURCES, epoch_source_hash())


# ---- libenvbuild_collect.so: the collection phase — the rollout buffer, truncation bootstraps, the episode log
# (include/envbuild_collect.h).  A fourth library of its own, built the way the second and third are; it includes no header of theirs. ----
COLLECT_LIB = os.path.join(HERE, 'lib', 'libenvbuild_collect.so')
COLLECT_SOURCES = ['eb_collect.hip']
COLLECT_HEADERS = ['eb_collect.h', 'eb_collect_device.h', os.path.join('..', '..', 'include', 'envbuild_collect.h'),
                   os.path.join('..', '..', 'include', 'envbuild.h')]


def collect_source_hash():
    """source_hash() of the collection library: the flags and the bytes of COLLECT_SOURCES and COLLECT_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in COLLECT_SOURCES + COLLECT_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def collect_needs_build():
    try:
        with open(COLLECT_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(COLLECT_LIB) or built != collect_source_hash()


def build_collect(force=False, verbose=False):
    """build() for libenvbuild_collect.so"""
    if not force and not collect_needs_build():
        return COLLECT_LIB
    import fcntl
    os.makedirs(os.path.dirname(COLLECT_LIB), exist_ok=True)
    with open(COLLECT_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not collect_needs_build():
            return COLLECT_LIB
        return _build_locked(verbose, COLLECT_LIB, COLLECT_SOURCES, collect_source_hash())


# ---- libenvbuild_ctl.so: the controls of the update phase on the device — the iteration's learning-rate factor and the approximate-KL
# stop (include/envbuild_ctl.h).  A fifth library of its own, built the way the other three small ones are.  Its unit takes the Adam
# element, its uniforms and the block fold from eb_train_device.h and eb_adam_args from envbuild_train.h, so those two headers are part of
# this library's hash too (and stay in TRAIN_HEADERS, unchanged). ----
CTL_LIB = os.path.join(HERE, 'lib', 'libenvbuild_ctl.so')
CTL_SOURCES = ['eb_ctl.hip']
CTL_HEADERS = ['eb_ctl.h', 'eb_ctl_device.h', os.path.join('..', '..', 'include', 'envbuild_ctl.h'),
               'eb_train_device.h', os.path.join('..', '..', 'include', 'envbuild_train.h'), os.path.join('..', '..', 'include', 'envbuild.h')]


def ctl_source_hash():
    """source_hash() of the control library: the flags and the bytes of CTL_SOURCES and CTL_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in CTL_SOURCES + CTL_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def ctl_needs_build():
    try:
        with open(CTL_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(CTL_LIB) or built != ctl_source_hash()


def build_ctl(force=False, verbose=False):
    """build() for libenvbuild_ctl.so"""
    if not force and not ctl_needs_build():
        return CTL_LIB
    import fcntl
    os.makedirs(os.path.dirname(CTL_LIB), exist_ok=True)
    with open(CTL_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not ctl_needs_build():
            return CTL_LIB
        return _build_locked(verbose, CTL_LIB, CTL_SOURCES, ctl_source_hash())


# ---- libenvbuild_ac.so: the two row kernels of a shared-trunk actor-critic — the PPO and value-loss rows with the whole cotangent, and
# the sampling row with the split (include/envbuild_ac.h).  A sixth library of its own, built the way the other four small ones are.  Its
# unit calls the row functions of eb_policy_logp_device.h (and, through it, eb_policy_sample_device.h, eb_mlp_device.h, eb_env_device.h
# and what they include) and of eb_train_device.h, so those headers are part of this library's hash too (and stay in HEADERS and
# TRAIN_HEADERS, unchanged). ----
AC_LIB = os.path.join(HERE, 'lib', 'libenvbuild_ac.so')
AC_SOURCES = ['eb_ac.hip']
AC_HEADERS = ['eb_ac.h', os.path.join('..', '..', 'include', 'envbuild_ac.h'),
              'eb_policy_logp_device.h', 'eb_policy_sample_device.h', 'eb_mlp_device.h', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h',
              'eb_train_device.h', os.path.join('..', '..', 'include', 'envbuild.h')]


def ac_source_hash():
    """source_hash() of the actor-critic library: the flags and the bytes of AC_SOURCES and AC_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in AC_SOURCES + AC_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def ac_needs_build():
    try:
        with open(AC_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(AC_LIB) or built != ac_source_hash()


def build_ac(force=False, verbose=False):
    """build() for libenvbuild_ac.so"""
    if not force and not ac_needs_build():
        return AC_LIB
    import fcntl
    os.makedirs(os.path.dirname(AC_LIB), exist_ok=True)
    with open(AC_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not ac_needs_build():
            return AC_LIB
        return _build_locked(verbose, AC_LIB, AC_SOURCES, ac_source_hash())


# ---- libenvbuild_norm.so: the running normalisation of observations and rewards — the batch sums, the merge into the running statistics
# and the normalisation (include/envbuild_norm.h).  A seventh library of its own, built the way the other five small ones are; it includes
# no header of theirs. ----
NORM_LIB = os.path.join(HERE, 'lib', 'libenvbuild_norm.so')
NORM_SOURCES = ['eb_norm.hip']
NORM_HEADERS = ['eb_norm.h', 'eb_norm_device.h', os.path.join('..', '..', 'include', 'envbuild_norm.h'),
                os.path.join('..', '..', 'include', 'envbuild.h')]


def norm_source_hash():
    """source_hash() of the normalisation library: the flags and the bytes of NORM_SOURCES and NORM_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in NORM_SOURCES + NORM_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def norm_needs_build():
    try:
        with open(NORM_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(NORM_LIB) or built != norm_source_hash()


def build_norm(force=False, verbose=False):
    """build() for libenvbuild_norm.so"""
    if not force and not norm_needs_build():
        return NORM_LIB
    import fcntl
    os.makedirs(os.path.dirname(NORM_LIB), exist_ok=True)
    with open(NORM_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not norm_needs_build():
            return NORM_LIB
        return _build_locked(verbose, NORM_LIB, NORM_SOURCES, norm_source_hash())


# ---- libenvbuild_offpolicy.so: off-policy training — the replay ring, the SAC critic and actor rows, the action gradient and the target
# averaging (include/envbuild_offpolicy.h).  An eighth library of its own, built the way the other six small ones are.  Its unit takes
# splitmix64 from eb_env_device.h and exp_det from eb_mlp_device.h, so those headers and what they include are part of this library's hash
# too (and stay in HEADERS, unchanged). ----
OFFPOLICY_LIB = os.path.join(HERE, 'lib', 'libenvbuild_offpolicy.so')
OFFPOLICY_SOURCES = ['eb_offpolicy.hip']
OFFPOLICY_HEADERS = ['eb_offpolicy.h', 'eb_offpolicy_device.h', os.path.join('..', '..', 'include', 'envbuild_offpolicy.h'),
                     'eb_mlp_device.h', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h', os.path.join('..', '..', 'include', 'envbuild.h')]


def offpolicy_source_hash():
    """source_hash() of the off-policy library: the flags and the bytes of OFFPOLICY_SOURCES and OFFPOLICY_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in OFFPOLICY_SOURCES + OFFPOLICY_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def offpolicy_needs_build():
    try:
        with open(OFFPOLICY_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(OFFPOLICY_LIB) or built != offpolicy_source_hash()


def build_offpolicy(force=False, verbose=False):
    """build() for libenvbuild_offpolicy.so"""
    if not force and not offpolicy_needs_build():
        return OFFPOLICY_LIB
    import fcntl
    os.makedirs(os.path.dirname(OFFPOLICY_LIB), exist_ok=True)
    with open(OFFPOLICY_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not offpolicy_needs_build():
            return OFFPOLICY_LIB
        return _build_locked(verbose, OFFPOLICY_LIB, OFFPOLICY_SOURCES, offpolicy_source_hash())


# ---- libenvbuild_per.so: prioritised experience replay — the radix-32 sum tree over the ring's slots, the stratified draw, the importance
# weights and the priority write-back (include/envbuild_per.h).  A ninth library of its own, built the way the other seven small ones are.
# Its unit takes the keyed word from eb_offpolicy_device.h, log_det from eb_policy_sample_device.h, exp_det from eb_mlp_device.h and
# splitmix64 from eb_env_device.h, so those headers and what they include are part of this library's hash too (and stay in HEADERS and
# OFFPOLICY_HEADERS, unchanged). ----
PER_LIB = os.path.join(HERE, 'lib', 'libenvbuild_per.so')
PER_SOURCES = ['eb_per.hip']
PER_HEADERS = ['eb_per.h', 'eb_per_device.h', os.path.join('..', '..', 'include', 'envbuild_per.h'),
               'eb_offpolicy_device.h', 'eb_policy_sample_device.h', 'eb_mlp_device.h', 'eb_env_device.h', 'eb_device.h', 'eb_kernels.h',
               os.path.join('..', '..', 'include', 'envbuild.h')]


def per_source_hash():
    """source_hash() of the prioritised-replay library: the flags and the bytes of PER_SOURCES and PER_HEADERS"""
    h = hashlib.sha256()
    h.update('\0'.join(FLAGS + ['|'] + LINK_FLAGS).encode())
    for f in PER_SOURCES + PER_HEADERS:
        h.update(b'\0' + f.encode() + b'\0')
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def per_needs_build():
    try:
        with open(PER_LIB + '.srchash') as fh:
            built = fh.read().strip()
    except OSError:
        built = None
    return not os.path.isfile(PER_LIB) or built != per_source_hash()


def build_per(force=False, verbose=False):
    """build() for libenvbuild_per.so"""
    if not force and not per_needs_build():
        return PER_LIB
    import fcntl
    os.makedirs(os.path.dirname(PER_LIB), exist_ok=True)
    with open(PER_LIB + '.lock', 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not per_needs_build():
            return PER_LIB
        return _build_locked(verbose, PER_LIB, PER_SOURCES, per_source_hash())


if __name__ == '__main__':
    print(build(force=True, verbose=True))
    print(build_train(force=True, verbose=True))
    print(build_epoch(force=True, verbose=True))
    print(build_collect(force=True, verbose=True))
    print(build_ctl(force=True, verbose=True))
    print(build_ac(force=True, verbose=True))
    print(build_norm(force=True, verbose=True))
    print(build_offpolicy(force=True, verbose=True))
    print(build_per(force=True, verbose=True))
