"""tools/call_trace.py: what the recorder writes for two host calls, and what diff reports. Needs no GPU."""
import importlib.util
import os

import numpy as np

import htm_hashjoin_amd as hj

_spec = importlib.util.spec_from_file_location(
    "call_trace", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "call_trace.py"))
call_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(call_trace)


def _two_calls():
    entries = []
    with call_trace.recording(hj.lib, entries.append):
        hj.key_hash_host(np.arange(5, dtype=np.uint64), key_mask=0xFF)
        hj.pairs_where_host(np.array([0, 1, 3], dtype=np.uint32), np.array([1, 0, 1], dtype=np.uint32), 0,
                            [(np.arange(4, dtype=np.int32), "<", np.arange(2, dtype=np.int32))], capacity=2, marks=False)
    return entries


def test_recording_yields_the_calls_with_their_scalars():
    # hj_key_hash_host(cols, n_cols, side, n_rows, key_mask, out); hj_pairs_where_host(map_s, map_r, n_pairs, s_row_base, s_rows,
    # r_rows, terms, n_terms, out_s, out_r, capacity, s_marks, r_marks, info)
    assert _two_calls() == ["hj_key_hash_host ptr 1 0 5 255 ptr",
                            "hj_pairs_where_host ptr ptr 3 0 4 2 ptr 1 ptr ptr 2 null null ptr"]


def test_recording_puts_the_functions_back():
    before = hj.lib.hj_key_hash_host
    _two_calls()
    assert hj.lib.hj_key_hash_host is before


def _trace(tmp_path, name, entries):
    path = tmp_path / name
    path.write_text("# tests/test_x.py::test_a\n" + "\n".join(entries) + "\n# tests/test_x.py::test_b\n" + entries[0] + "\n")
    return call_trace.read_trace(str(path))


def test_diff_of_a_trace_with_itself_is_empty(tmp_path):
    a = _trace(tmp_path, "a.txt", _two_calls())
    assert list(a) == ["", "tests/test_x.py::test_a", "tests/test_x.py::test_b"] and len(a["tests/test_x.py::test_a"]) == 2
    assert call_trace.diff(a, a) == []


def test_diff_names_the_entry_whose_scalar_changed(tmp_path):
    entries = _two_calls()
    changed = [entries[0], entries[1].replace(" ptr 2 null", " ptr 3 null")]
    assert changed != entries
    report = call_trace.diff(_trace(tmp_path, "a.txt", entries), _trace(tmp_path, "b.txt", changed))
    assert len(report) == 1
    assert report[0].startswith("tests/test_x.py::test_a: call 1 of 2 / 2 differs")
    assert "A: " + entries[1] in report[0] and "B: " + changed[1] in report[0]


def test_diff_leaves_the_memory_calls_out_of_the_sequence_and_reports_what_rose(tmp_path):
    entries = _two_calls()
    fewer = ["hj_dev_alloc ptr 64 ptr", "hj_copy_h2d ptr ptr ptr 64"] + entries
    more = ["hj_dev_alloc ptr 64 ptr", "hj_copy_h2d ptr ptr ptr 64", "hj_copy_h2d ptr ptr ptr 8"] + entries
    a, b = _trace(tmp_path, "a.txt", fewer), _trace(tmp_path, "b.txt", more)
    assert call_trace.diff(b, a) == []          # planes that disappear are no difference
    assert call_trace.diff(a, b) == ["tests/test_x.py::test_a: memory calls 2 -> 3, bytes copied 64 -> 72"]
