"""CPU: every entry of include/*.h that takes a `void* stream` is accounted for — a row of tests/_capture_cases.CAPTURED (issued on a side
stream, captured and replayed by tests/test_gpu_capture.py) or a member of NOT_CAPTURED with the reason.  An entry that joins the ABI
makes this fail until someone has decided which."""
import os
import shutil

from tests._capture_cases import CAPTURED, NOT_CAPTURED, ROOT, Row, entries_of, stream_entries


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
