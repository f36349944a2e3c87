"""CPU (-m "not gpu"): every optional family of the C ABI (_capi.FAMILIES, one public header each) is declared as ctypes binds it,
exported by the built library next to a gfx950 kernel, kept out of the hashed forward sources, refuses NULL handles by name without
a device and is refused by name by a library without it; every ABI number is the pinned one.  One test per property, parametrised
over the product's table; ROWS holds what that table does not."""
import ctypes as C
import os
import re

import pytest

from env_build_amd import _capi, build as eb_build
from tests._helpers import ROOT, oracle_lib


def row(kernels, units, headers, attrs, entries=None, n_args=None, says=(), no_hashed_source_has=(), unhashed=(), macros=None, null_calls=()):
    return dict(kernels=kernels, units=units, headers=headers, attrs=attrs, entries=entries, n_args=n_args or {}, says=says,
                no_hashed_source_has=no_hashed_source_has, unhashed=unhashed, macros=macros or {}, null_calls=null_calls)


def null(entry, *args, says=None):
    """one call with NULL handles: a ctypes type among the arguments stands for an output of that type holding 7.  The call returns -1,
    eb_last_error() contains `says` (by default "<entry>: null handle") and every output still holds 7"""
    return entry, args, says or entry + ': null handle'


# family -> kernel symbols expected in the library's code object, translation units (in build.SOURCES), private headers (in
# build.HEADERS), the CApi attributes a library without the family refuses, and the family's own pins: the exact sorted entry list,
# argument counts, what its public header says, a word no hashed forward source's name may carry, further files no hashed source list
# may hold, header #defines with their Python twin and its ceiling, and the refusals that need no device
ROWS = {
    'grad': row(('rollout_step_vjp_kernel',), ('eb_rollout_vjp.hip',), (),             # (its tape entries: tests/test_tape_grad_host.py)
                ('rollout_step_vjp', 'rollout_chain_vjp', 'grad_abi_version')),
    'cand': row(('rollout_tape_cand_kernel',), ('eb_rollout_tape_cand.hip',), ('eb_cand.h',),
                ('rollout_tape_cand', 'rollout_tape_cand_max', 'cand_abi_version')),
    'cand_grad': row(('rollout_tape_cand_vjp_kernel',), ('eb_rollout_tape_cand_vjp.hip',), ('eb_cand_grad.h',),
                     ('rollout_tape_cand_vjp', 'rollout_tape_cand_vjp_max', 'cand_grad_abi_version'),
                     says=('g_out5_steps', 'g_obs_final', 'eb_rollout_tape_cand'), no_hashed_source_has=('cand',)),
    'sample': row(('rollout_tape_sample_kernel',), ('eb_rollout_tape_sample.hip',), ('eb_sample.h',),
                  ('rollout_tape_sample', 'rollout_tape_sample_max', 'sample_abi_version'), n_args={'eb_rollout_tape_sample': 22}),
    'ilqr': row(('rollout_tape_ilqr_kernel',), ('eb_rollout_tape_ilqr.hip',), ('eb_ilqr.h', 'eb_ilqr_device.h'),
                ('rollout_tape_ilqr', 'rollout_tape_ilqr_max', 'ilqr_abi_version'), n_args={'eb_rollout_tape_ilqr': 23}),
    'mlp_f16': row(('mlp_f16_kernel',), ('eb_policy_f16.hip',), ('eb_policy_f16.h',),
                   ('mlp_set_precision', 'mlp_get_precision', 'mlp_f16_abi_version'),
                   says=('round-to-nearest-even', 'subnormal', 'NOT part of the contract', 'mlp_f16_reference'),
                   macros={'EB_MLP_PRECISION_F32': (_capi.MLP_PRECISION_ID['fp32'], 0), 'EB_MLP_PRECISION_F16': (_capi.MLP_PRECISION_ID['fp16'], 1)},
                   null_calls=(null('eb_mlp_set_precision', None, 1), null('eb_mlp_get_precision', None, C.c_int32))),
    'policy_rollout': row(('policy_rollout_kernel', 'mlp_f16_kernel'), ('eb_policy_rollout.hip',), ('eb_policy_rollout.h', 'eb_policy_f16_device.h'),
                          ('policy_rollout', 'policy_rollout_supported', 'policy_rollout_abi_version'),
                          entries=['eb_policy_rollout', 'eb_policy_rollout_abi_version', 'eb_policy_rollout_supported'],
                          n_args={'eb_policy_rollout': 16, 'eb_policy_rollout_supported': 3},
                          says=('bit for bit', 'eb_policy_run_batch', 'eb_rollout_step', 'ALWAYS one launch', 'AFTER step t'),
                          null_calls=(null('eb_policy_rollout_supported', None, None, C.c_int32, says='eb_policy_rollout_supported'),
                                      null('eb_policy_rollout', None, None, 4, 5, None, None, 0, 1.0, 0, None, None, None, None, None, None, None))),
    'mlp_grad': row(('mlp_bwd_data_kernel', 'mlp_wgrad_kernel', 'mlp_wgrad_reduce_kernel', 'mlp_pack_kernel'), ('eb_policy_grad.hip',),
                    ('eb_policy_grad.h',),
                    ('mlp_backward', 'mlp_set_params_device', 'mlp_grad_supported', 'mlp_param_count', 'mlp_backward_workspace_bytes',
                     'mlp_grad_abi_version'),
                    entries=['eb_mlp_backward', 'eb_mlp_backward_workspace_bytes', 'eb_mlp_grad_abi_version', 'eb_mlp_grad_supported',
                             'eb_mlp_param_count', 'eb_mlp_set_params_device'],
                    n_args={'eb_mlp_backward': 12},
                    says=('NOT part of the contract', 'mlp_backward_reference', 'non-finite', 'bit for bit', 'y > 0 ? 1 : y + 1', 'EB_ESTATE',
                          'Model.get_weights()'),
                    null_calls=(null('eb_mlp_grad_supported', None, C.c_int32), null('eb_mlp_param_count', None, C.c_int64),
                                null('eb_mlp_set_params_device', None, None, None), null('eb_mlp_backward_workspace_bytes', None, 4, C.c_size_t),
                                null('eb_mlp_backward', None, 4, None, None, 0, 1.0, None, 0, None, None, None, None))),
    'policy_rollout_grad': row(('policy_rollout_grad_kernel', 'mlp_wgrad_kernel'), ('eb_policy_rollout_grad.hip',),
                               ('eb_policy_rollout_grad.h', 'eb_mlp_device.h'),
                               ('policy_rollout_grad', 'policy_rollout_grad_abi_version', 'policy_rollout_grad_supported',
                                'policy_rollout_grad_workspace_bytes'),
                               entries=['eb_policy_rollout_grad', 'eb_policy_rollout_grad_abi_version', 'eb_policy_rollout_grad_supported',
                                        'eb_policy_rollout_grad_workspace_bytes'],
                               n_args={'eb_policy_rollout_grad': 20, 'eb_policy_rollout_grad_abi_version': 0, 'eb_policy_rollout_grad_supported': 3,
                                       'eb_policy_rollout_grad_workspace_bytes': 5},
                               says=('bit for bit', 'eb_rollout_step_vjp', 'eb_mlp_backward', 'HOST pointer', 'multiple of 64', 'never another code path'),
                               unhashed=('eb_policy_grad.hip', 'eb_policy_grad.h', 'eb_capi.hip'),
                               macros={'EB_POLICY_ROLLOUT_GRAD_MAX_STEPS': (_capi.POLICY_ROLLOUT_GRAD_MAX_STEPS, 128)},
                               null_calls=(null('eb_policy_rollout_grad_supported', None, None, C.c_int32),
                                           null('eb_policy_rollout_grad_workspace_bytes', None, None, 4, 5, C.c_size_t),
                                           null('eb_policy_rollout_grad', None, None, 4, 5, None, None, 0, 1.0, None, None, 0, *([None] * 9)))),
}
# family (None: envbuild.h itself) -> (header, pinned EB_*_ABI_VERSION)
ABI_NUMBERS = {None: ('envbuild.h', 5), 'grad': ('envbuild_grad.h', 2), 'cand': ('envbuild_cand.h', 1), 'cand_grad': ('envbuild_cand_grad.h', 1),
               'sample': ('envbuild_sample.h', 1), 'ilqr': ('envbuild_ilqr.h', 1), 'mlp_f16': ('envbuild_mlp_f16.h', 1),
               'policy_rollout': ('envbuild_policy_rollout.h', 1), 'mlp_grad': ('envbuild_mlp_grad.h', 1),
               'policy_rollout_grad': ('envbuild_policy_rollout_grad.h', 1)}
FAMILY_NAMES = list(_capi.FAMILIES)


def header_text(header):
    return open(os.path.join(ROOT, 'include', header)).read()


def macro(family):
    return 'EB_%sABI_VERSION' % ('' if family is None else family.upper() + '_')


def defined(name, header):
    return int(re.search(r'#define %s (\d+)' % name, header_text(header)).group(1))


def test_abi_numbers():
    assert list(ABI_NUMBERS) == [None] + FAMILY_NAMES == [None] + list(ROWS)
    assert FAMILY_NAMES == ['grad', 'cand', 'cand_grad', 'sample', 'ilqr', 'mlp_f16', 'policy_rollout', 'mlp_grad', 'policy_rollout_grad']
    for family, (header, want) in ABI_NUMBERS.items():
        assert getattr(_capi, macro(family)) == want, macro(family)
        assert defined(macro(family), header) == want, header
        if family is not None:
            fam = _capi.FAMILIES[family]
            assert len(fam) == 6 and fam[0] == header and fam[4] == want and fam[3] == 'eb_%s_abi_version' % family and fam[3] in fam[5]
            assert isinstance(fam[1], str) and isinstance(fam[2], str)
            assert getattr(_capi.CApi, family + '_fn')
    assert _capi.MLP_PRECISION_ID == {'fp32': 0, 'fp16': 1}
    for missing in ('no_such_family', 'mlp_grad_f16'):
        with pytest.raises(KeyError):
            _capi.FAMILIES[missing]
    assert _capi.CApi.family_fn.__doc__
    # one table: the names of the tables it replaced are gone, so a stale import fails loudly
    for gone in ('MORE_FAMILIES', 'POLICY_FAMILIES', 'TRAIN_FAMILIES', 'LOOP_GRAD_FAMILIES', '_FAMILY_TABLES', '_ALL_FAMILY_TABLES', 'family_row'):
        assert not hasattr(_capi, gone), gone


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_header_declares_what_ctypes_binds(family):
    header, _label, _abi, version_symbol, version, prototypes = _capi.FAMILIES[family]
    mine = ROWS[family]
    text = header_text(header)
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert sorted(prototypes) == sorted(set(re.findall(r'\b(eb_[a-z0-9_]+)\s*\(', src)))
    assert mine['entries'] is None or sorted(prototypes) == mine['entries']
    for name, (_res, args) in prototypes.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
        assert m, '%s is not declared in include/%s' % (name, header)
        declared = [a for a in m.group(1).split(',') if a.strip() != 'void']
        assert len(declared) == len(args), name
    for name, n in mine['n_args'].items():
        assert len(prototypes[name][1]) == n, name
    # a table of its own: envbuild.h's set is the oracle's too, every other family's is bound by itself
    assert prototypes is getattr(_capi, family.upper() + '_PROTOTYPES') and version_symbol in prototypes
    assert not set(prototypes) & set(_capi.PROTOTYPES)
    for other in FAMILY_NAMES:
        assert other == family or not set(prototypes) & set(_capi.FAMILIES[other][5]), other
    assert version == getattr(_capi, macro(family)) == defined(macro(family), header) == ABI_NUMBERS[family][1]
    for name, (twin, most) in mine['macros'].items():
        assert defined(name, header) == twin <= most, name
    for words in mine['says']:
        assert words in text, words


@pytest.fixture(scope='module')
def hip_library():
    lib_path = eb_build.build()            # hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
    import torch  # noqa: F401  (binds the HIP runtime torch ships before ours, as the product does)
    lib = C.CDLL(lib_path)
    lib.eb_last_error.restype = C.c_char_p
    return lib, open(lib_path, 'rb').read()


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_hip_library_exports_the_entries_and_a_gfx950_kernel(family, hip_library):
    lib, blob = hip_library
    header, _label, _abi, version_symbol, _version, prototypes = _capi.FAMILIES[family]
    mine = ROWS[family]
    for name in prototypes:
        assert hasattr(lib, name), name
    assert getattr(lib, version_symbol)() == ABI_NUMBERS[family][1]
    assert b'gfx950' in blob
    for kernel in mine['kernels']:
        assert kernel.encode() in blob, kernel
    public = os.path.join('..', '..', 'include', header)
    assert set(mine['units']) <= set(eb_build.SOURCES) and set(mine['headers'] + (public,)) <= set(eb_build.HEADERS)
    for f in eb_build.SOURCES + eb_build.HEADERS:
        assert os.path.isfile(os.path.join(eb_build.CSRC, f)), f
    # translation units of its own: the forward kernels' hashes (profiles/ ties HBM-traffic records to them) do not see the family
    for files in eb_build.KERNEL_SOURCES.values():
        assert not set(files) & set(mine['units'] + mine['headers'] + (public,) + mine['unhashed'])
        assert not [f for f in files for word in mine['no_hashed_source_has'] if word in f]
    # the refusals of NULL handles need no device: the handles are checked first, and each entry names itself
    for name, args, says in mine['null_calls']:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = prototypes[name]
        outs = [a(7) for a in args if isinstance(a, type)]
        filled = iter(outs)
        assert fn(*[C.byref(next(filled)) if isinstance(a, type) else a for a in args]) == -1, name
        assert says.encode() in lib.eb_last_error(), name
        assert all(out.value == 7 for out in outs), name


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_a_library_without_the_family_is_refused_cleanly(family):
    """on the oracle library, which exports none of the optional families, the entries this table names are refused with the family's own
    label and header through __getattr__, the family's one-line method and family_fn alike (every symbol of every row:
    tests/test_abi_and_host.py)"""
    api = oracle_lib()                     # CApi binds every PROTOTYPES entry on it, as before
    assert api.backend == 'oracle'
    header, label, _abi, _version_symbol, _version, prototypes = _capi.FAMILIES[family]
    assert os.path.isfile(os.path.join(ROOT, 'include', header))
    for name in ROWS[family]['attrs']:
        assert 'eb_' + name in prototypes and not hasattr(api.lib, 'eb_' + name), name
        for refused in (lambda: getattr(api, name), lambda: getattr(api, family + '_fn')('eb_' + name), lambda: api.family_fn(family, 'eb_' + name)):
            with pytest.raises(_capi.EbError) as e:
                refused()
            assert label in str(e.value) and header in str(e.value), name
