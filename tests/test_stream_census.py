"""CPU: every entry of include/*.h that takes a `void* stream` is accounted for — a row of tests/_capture_cases.CAPTURED (issued on a side
stream, captured and replayed by tests/test_gpu_capture.py) or a member of NOT_CAPTURED with the reason.  An entry that joins the ABI
makes this fail until someone has decided which.  The entries whose stream is a field of their argument struct are held the same way
against STRUCT_STREAM_HELD: each names the GPU test that runs it on a side stream and under capture."""
import os
import re
import shutil

from tests._capture_cases import (CAPTURED, NOT_CAPTURED, ROOT, STRUCT_STREAM_HELD, Row, entries_of, stream_entries, struct_stream_entries,
                                  function_text)


def captured_entries():
    return {e for key in CAPTURED for e in entries_of(key)}


def test_every_stream_taking_entry_is_in_exactly_one_set():
    declared = set(stream_entries())
    assert len(declared) == 50, sorted(declared)
    assert declared == captured_entries() | set(NOT_CAPTURED), (sorted(declared - captured_entries() - set(NOT_CAPTURED)),
                                                                 sorted((captured_entries() | set(NOT_CAPTURED)) - declared))
    assert not captured_entries() & set(NOT_CAPTURED)
    assert all(isinstance(why, str) and why.strip() for why in NOT_CAPTURED.values())
    for name in ('eb_rollout_gated', 'eb_gate_feed', 'eb_plan_launch', 'eb_event_record'):
        assert name in NOT_CAPTURED


def test_the_parser_sees_a_new_entry_and_skips_comments(tmp_path):
    inc = tmp_path / 'include'
    shutil.copytree(os.path.join(ROOT, 'include'), str(inc))
    with open(str(inc / 'envbuild_cand.h'), 'a') as fh:
        fh.write('\n/* int eb_in_a_comment(void* stream); */\n// int eb_in_a_line_comment(void* stream);\n'
                 'int eb_x(void* stream);\nint eb_no_stream(int32_t n);\n'
                 'int eb_y(eb_handle h, const float* a,\n         float* b, void *stream);\n')
    found = stream_entries(str(inc))
    assert set(found) - set(stream_entries()) == {'eb_x', 'eb_y'}
    assert found['eb_y'] == [(False, 'h'), (True, 'a'), (False, 'b'), (False, 'stream')]
    assert set(found) != captured_entries() | set(NOT_CAPTURED)


def test_rows_are_well_formed():
    for key, r in CAPTURED.items():
        assert isinstance(r, Row) and callable(r.make) and r.sizes, key
        assert r.kernels is None or callable(r.kernels) or isinstance(r.kernels, int) or (
            isinstance(r.kernels, tuple) and r.kernels[1] in CAPTURED), key
        if r.kernels is None:        # a measured count is held equal at two batch sizes
            rest = lambda s: tuple(sorted((k, v) for k, v in s.items() if k != 'n'))
            for s in r.sizes:
                assert len({t['n'] for t in r.sizes if rest(t) == rest(s)}) >= 2, key
        for kind, why in r.other_nodes:
            assert kind in ('memset', 'memcpy') and why.strip(), key


def test_every_struct_taking_entry_with_a_stream_field_names_its_capture_test():
    declared = struct_stream_entries()
    assert len(declared) == 20 and not set(declared) & set(stream_entries()), sorted(declared)
    assert set(declared) == set(STRUCT_STREAM_HELD), (sorted(set(declared) - set(STRUCT_STREAM_HELD)), sorted(set(STRUCT_STREAM_HELD) - set(declared)))
    assert declared['eb_adam_step_ctl'] == 'eb_adam_ctl_args' and declared['eb_adam_step'] == 'eb_adam_args'      # nested / direct
    for entry, (module, name) in STRUCT_STREAM_HELD.items():
        assert module.startswith('test_gpu_') and name.startswith('test_'), entry
        text = function_text(module, name)
        assert text is not None, '%s: tests/%s.py has no function %s' % (entry, module, name)
        assert re.search(r"['\"]%s['\"]" % entry, text), '%s is not mentioned by %s.%s' % (entry, module, name)
        assert 'side' in text and re.search(r'\bcapture\(', text) and 'replay' in text, (entry, module, name)
    assert function_text('test_gpu_ctl', 'test_no_such_function') is None


def test_the_struct_parser_sees_a_new_entry_direct_or_nested(tmp_path):
    inc = tmp_path / 'include'
    shutil.copytree(os.path.join(ROOT, 'include'), str(inc))
    with open(str(inc / 'envbuild_ctl.h'), 'a') as fh:
        fh.write('\ntypedef struct eb_new_args {\n    int32_t n;   /* void* stream; in a comment */\n    void* stream;\n} eb_new_args;\n'
                 'typedef struct eb_outer_args { eb_new_args inner; float lr; } eb_outer_args;\n'
                 'typedef struct eb_plain_args { int32_t n; const float* x; } eb_plain_args;\n'
                 'int eb_new(const eb_new_args* a);\nint eb_outer(eb_mlp m, const eb_outer_args *a);\nint eb_plain(const eb_plain_args* a);\n'
                 '// int eb_commented(const eb_new_args* a);\n')
    found = struct_stream_entries(str(inc))
    assert set(found) - set(struct_stream_entries()) == {'eb_new', 'eb_outer'}
    assert found['eb_outer'] == 'eb_outer_args' and set(found) != set(STRUCT_STREAM_HELD)
