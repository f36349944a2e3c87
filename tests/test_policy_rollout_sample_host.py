"""CPU (-m "not gpu"): the stochastic closed-loop rollout (include/envbuild_policy_rollout_sample.h, env_build_amd.policy_rollout) — its
header against the module's own binding table and argument struct (every field's offset as the host compiler lays the C struct out),
the built library's exports, device-free refusals, and the stream census, which this family leaves as it was."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from env_build_amd import _capi, build as eb_build
from env_build_amd import policy_rollout as pr
from tests._capture_cases import stream_entries
from tests._helpers import ROOT, oracle_lib

HEADER = os.path.join(ROOT, 'include', 'envbuild_policy_rollout_sample.h')
ENTRIES = ['eb_policy_rollout_sample', 'eb_policy_rollout_sample_abi_version', 'eb_policy_rollout_sample_supported',
           'eb_policy_rollout_sample_workspace_bytes']
FIELDS = ['struct_size', 'n_env', 'steps', 'path_id', 'action_range', 'w_logp', 'w5', 'seed', 'counter', 'obs_in', 'ref_idx', 'row_ids',
          'eps_steps', 'workspace', 'workspace_bytes', 'obs_out', 'out5_steps', 'actions_steps', 'obs_steps', 'cost', 'logp_steps',
          'eps_out_steps', 'g_actions_steps', 'g_obs0', 'g_params', 'stream']


def test_header_declares_what_the_module_binds():
    text = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES) == sorted(set(re.findall(r'\b(eb_policy_rollout_sample\w*)\s*\(', src))) == ENTRIES
    for name, (_res, args) in pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, name
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert {n: len(a) for n, (_r, a) in pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES.items()} == {
        'eb_policy_rollout_sample_abi_version': 0, 'eb_policy_rollout_sample_supported': 3, 'eb_policy_rollout_sample_workspace_bytes': 6,
        'eb_policy_rollout_sample': 3}
    assert int(re.search(r'#define EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION (\d+)', text).group(1)) == pr.EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION == 1
    assert int(re.search(r'#define EB_POLICY_ROLLOUT_SAMPLE_MAX_STEPS (\d+)', text).group(1)) == pr.POLICY_ROLLOUT_SAMPLE_MAX_STEPS == 128
    body = re.search(r'typedef struct eb_policy_rollout_sample_args \{(.*?)\} eb_policy_rollout_sample_args;', src, flags=re.S).group(1)
    declared = [n for stmt in body.split(';') for n in re.findall(r'(\w+)\s*(?:\[\d+\])?\s*(?:,|$)', stmt.strip())]
    assert declared == FIELDS == [f[0] for f in pr.RolloutSampleArgs._fields_]
    for words in ('bit for bit', 'AT CALL TIME', 'tests/test_stream_census.py', 'exactly three', 'needs NONE', 'head 0', 'counter + t'):
        assert words in text, words


def test_the_struct_is_laid_out_as_the_host_compiler_lays_it_out(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/llvm/bin/clang'
    src = tmp_path / 'layout.c'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "envbuild_policy_rollout_sample.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(eb_policy_rollout_sample_args));']
    lines += ['  printf("%s %%zu\\n", offsetof(eb_policy_rollout_sample_args, %s));' % (f, f) for f in FIELDS]
    lines += ['  return 0;', '}']
    src.write_text('\n'.join(lines) + '\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe])
    out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(out.pop('sizeof')) == C.sizeof(pr.RolloutSampleArgs)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(pr.RolloutSampleArgs, f).offset for f in FIELDS}
    a = pr.sample_args(n_env=3, w5=(1, 2, 3, 4, 5))
    assert a.struct_size == C.sizeof(pr.RolloutSampleArgs) and list(a.w5) == [1.0, 2.0, 3.0, 4.0, 5.0] and a.obs_in is None


def test_the_family_tables_and_the_stream_census_are_untouched():
    assert list(_capi.FAMILIES) == ['grad', 'cand', 'cand_grad', 'sample', 'ilqr', 'mlp_f16', 'policy_rollout', 'mlp_grad',
                                    'policy_rollout_grad']
    assert not set(pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES) & set(_capi.PROTOTYPES)
    for row in _capi.FAMILIES.values():
        assert not set(pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES) & set(row[5])
    declared = stream_entries()
    assert len(declared) == 50 and not [n for n in declared if n.startswith('eb_policy_rollout_sample')]


@pytest.fixture(scope='module')
def hip_library():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    lib.eb_last_error.restype = C.c_char_p
    for name, (res, args) in pr.POLICY_ROLLOUT_SAMPLE_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib, open(lib_path, 'rb').read()


def test_the_library_exports_the_entries_and_the_kernel(hip_library):
    lib, blob = hip_library
    assert lib.eb_policy_rollout_sample_abi_version() == 1
    assert b'gfx950' in blob and b'policy_rollout_sample_kernel' in blob
    public = os.path.join('..', '..', 'include', 'envbuild_policy_rollout_sample.h')
    assert 'eb_policy_rollout_sample.hip' in eb_build.SOURCES
    assert {'eb_policy_rollout_sample.h', public} <= set(eb_build.HEADERS)
    for files in eb_build.KERNEL_SOURCES.values():
        assert not [f for f in files if 'policy_rollout_sample' in f]


def test_refusals_need_no_device_and_name_their_entry(hip_library):
    lib, _ = hip_library
    seven, size = C.c_int32(7), C.c_size_t(7)
    fake = C.addressof((C.c_char * 64)())              # a non-NULL handle: the checks below stop before either handle is looked at
    good, short = pr.sample_args(n_env=4, steps=5), pr.sample_args(n_env=4, steps=5)
    short.struct_size = C.sizeof(pr.RolloutSampleArgs) - 8
    calls = [
        ('eb_policy_rollout_sample_supported', (None, fake, C.byref(seven)), 'null handle'),
        ('eb_policy_rollout_sample_supported', (fake, None, C.byref(seven)), 'null policy'),
        ('eb_policy_rollout_sample_workspace_bytes', (None, fake, 4, 5, 1, C.byref(size)), 'null handle'),
        ('eb_policy_rollout_sample_workspace_bytes', (fake, None, 4, 5, 1, C.byref(size)), 'null policy'),
        ('eb_policy_rollout_sample', (None, fake, C.byref(good)), 'null handle'),
        ('eb_policy_rollout_sample', (fake, None, C.byref(good)), 'null policy'),
        ('eb_policy_rollout_sample', (fake, fake, None), 'null args'),
        ('eb_policy_rollout_sample', (fake, fake, C.byref(short)), 'struct_size is %d' % short.struct_size),
    ]
    for name, args, why in calls:
        assert getattr(lib, name)(*args) == -1, (name, why)
        err = lib.eb_last_error()
        assert err.startswith(name.encode() + b':') and why.encode() in err, (name, err)
    assert seven.value == 7 and size.value == 7


def test_a_library_without_the_entries_is_refused_by_header_name():
    api = oracle_lib()
    assert api.backend == 'oracle'
    with pytest.raises(_capi.EbError) as e:
        pr.bind_sample(api)
    assert 'envbuild_policy_rollout_sample.h' in str(e.value) and 'eb_policy_rollout_sample_workspace_bytes' in str(e.value)
