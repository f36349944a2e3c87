"""CPU (-m "not gpu"): the closed-loop rollout family (include/envbuild_policy_rollout.h) is declared as ctypes binds it, lives in a
third family table next to _capi.FAMILIES and _capi.MORE_FAMILIES (neither of which grows), is exported by the built library next to a
gfx950 policy_rollout_kernel, stays out of the hashed forward sources, refuses NULL handles by name without a device and is refused by
name by the oracle library."""
import ctypes as C
import os
import re

import pytest

from env_build_amd import _capi, build as eb_build
from tests._helpers import ROOT, oracle_lib

HEADER = 'envbuild_policy_rollout.h'
ALL_FAMILIES = ['grad', 'cand', 'cand_grad', 'sample', 'ilqr', 'mlp_f16', 'policy_rollout']


def header_src():
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    return text, re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_declares_what_ctypes_binds():
    text, src = header_src()
    protos = _capi.POLICY_ROLLOUT_PROTOTYPES
    assert sorted(protos) == sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert sorted(protos) == ['eb_policy_rollout', 'eb_policy_rollout_abi_version', 'eb_policy_rollout_supported']
    for name, (_res, args) in protos.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/%s' % (name, HEADER)
        assert len([a for a in m.group(1).split(',') if a.strip() != 'void']) == len(args), name
    assert len(protos['eb_policy_rollout'][1]) == 16 and len(protos['eb_policy_rollout_supported'][1]) == 3
    assert int(re.search(r'#define EB_POLICY_ROLLOUT_ABI_VERSION (\d+)', src).group(1)) == _capi.EB_POLICY_ROLLOUT_ABI_VERSION == 1
    assert not set(protos) & set(_capi.PROTOTYPES)
    for table in (_capi.FAMILIES, _capi.MORE_FAMILIES):
        for row in table.values():
            assert not set(protos) & set(row[5])
    for words in ('bit for bit', 'eb_policy_run_batch', 'eb_rollout_step', 'ALWAYS one launch', 'AFTER step t'):
        assert words in text, words


def test_the_third_family_table():
    assert list(_capi.FAMILIES) == ['grad', 'cand', 'cand_grad', 'sample', 'ilqr']            # neither of the first two grew
    assert list(_capi.MORE_FAMILIES) == ['mlp_f16']
    assert list(_capi.POLICY_FAMILIES) == ['policy_rollout']
    row = _capi.POLICY_FAMILIES['policy_rollout']
    assert len(row) == 6 == len(_capi.FAMILIES['grad']) == len(_capi.MORE_FAMILIES['mlp_f16'])
    assert row[0] == HEADER and row[3] == 'eb_policy_rollout_abi_version' and row[4] == 1 and row[5] is _capi.POLICY_ROLLOUT_PROTOTYPES
    tables = (_capi.FAMILIES, _capi.MORE_FAMILIES, _capi.POLICY_FAMILIES)
    assert [f for t in tables for f in t] == ALL_FAMILIES
    for family in ALL_FAMILIES:
        assert _capi.family_row(family) is next(t[family] for t in tables if family in t)
        assert len(_capi.family_row(family)) == 6
    with pytest.raises(KeyError):
        _capi.family_row('no_such_family')
    assert _capi.CApi.policy_rollout_fn


def test_hip_library_exports_the_entries_and_a_gfx950_kernel():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib, blob = C.CDLL(lib_path), open(lib_path, 'rb').read()
    for name in _capi.POLICY_ROLLOUT_PROTOTYPES:
        assert hasattr(lib, name), name
    assert lib.eb_policy_rollout_abi_version() == 1
    assert b'gfx950' in blob and b'policy_rollout_kernel' in blob and b'mlp_f16_kernel' in blob
    public = os.path.join('..', '..', 'include', HEADER)
    new = {'eb_policy_rollout.hip', 'eb_policy_rollout.h', 'eb_policy_f16_device.h', public}
    assert 'eb_policy_rollout.hip' in eb_build.SOURCES and {'eb_policy_rollout.h', 'eb_policy_f16_device.h', public} <= set(eb_build.HEADERS)
    for f in eb_build.SOURCES + eb_build.HEADERS:
        assert os.path.isfile(os.path.join(eb_build.CSRC, f)), f
    for files in eb_build.KERNEL_SOURCES.values():
        assert not set(files) & new
    # the refusals need no device: the handles are checked first
    lib.eb_last_error.restype = C.c_char_p
    ok = C.c_int32(7)
    assert lib.eb_policy_rollout_supported(None, None, C.byref(ok)) == -1 and ok.value == 7
    assert b'eb_policy_rollout_supported' in lib.eb_last_error()
    lib.eb_policy_rollout.argtypes = _capi.POLICY_ROLLOUT_PROTOTYPES['eb_policy_rollout'][1]
    assert lib.eb_policy_rollout(None, None, 4, 5, None, None, 0, 1.0, 0, None, None, None, None, None, None, None) == -1
    assert b'eb_policy_rollout: null handle' in lib.eb_last_error()


def test_the_oracle_library_is_refused_with_the_family_label_and_header():
    api = oracle_lib()
    assert api.backend == 'oracle'
    header, label = _capi.POLICY_FAMILIES['policy_rollout'][:2]
    assert header == HEADER
    for name in ('policy_rollout', 'policy_rollout_supported', 'policy_rollout_abi_version'):
        assert 'eb_' + name in _capi.POLICY_ROLLOUT_PROTOTYPES
        with pytest.raises(_capi.EbError) as e:
            getattr(api, name)
        assert label in str(e.value) and header in str(e.value), name
        for fn in (api.policy_rollout_fn, lambda s: api.family_fn('policy_rollout', s)):
            with pytest.raises(_capi.EbError) as e:
                fn('eb_' + name)
            assert label in str(e.value) and header in str(e.value), name
    assert not hasattr(api.lib, 'eb_policy_rollout')
    # the other families still resolve through the tables they were in
    with pytest.raises(_capi.EbError) as e:
        api.mlp_set_precision
    assert _capi.MORE_FAMILIES['mlp_f16'][1] in str(e.value)
