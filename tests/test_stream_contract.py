"""The "Stream contract" table of INTEGRATION.md against the ctypes prototypes of _lib.py: every exported hj_* entry point
appears exactly once with a known class, so a new entry point cannot ship unclassified, and the table names nothing that
does not exist. No GPU: the table is text, the prototypes a dict. tests/test_gpu_stream_order.py reads the asynchronous set
from the same table (stream_order.asynchronous_calls) for its pending() assertions."""
import os

import pytest

from htm_hashjoin_amd._lib import lib

import stream_order as so


def test_every_entry_point_is_classified_once():
    table = so.contract()                                   # raises on a name that appears twice
    declared = set(lib._hj_signatures)
    assert declared - set(table) == set(), ("entry points without a row", sorted(declared - set(table)))
    assert set(table) - declared == set(), ("rows without an entry point", sorted(set(table) - declared))
    unknown = {n: cls for n, (cls, _note) in table.items() if cls not in so.CLASSES}
    assert not unknown, unknown


def test_the_classes_the_gpu_tests_rely_on():
    """the delayed sequences assert pending() only over calls of the asynchronous class; these are the calls they are made of,
    and the calls the sequences leave that assertion out for"""
    a = so.asynchronous_calls()
    for name in ("hj_build_dev", "hj_probe_dev", "hj_probe_pairs_dev", "hj_probe_join_dev", "hj_r_rows_dev", "hj_gather_dev",
                 "hj_gather2_dev", "hj_prj_build_dev", "hj_prj_probe_dev", "hj_prj_probe_pairs_dev", "hj_prj_probe_join_dev",
                 "hj_prj_agg_begin", "hj_prj_probe_agg_dev", "hj_prj_agg_rows_dev", "hj_pairs_agg_dev", "hj_key_hash2_dev",
                 "hj_pairs_verify2_dev"):
        assert name in a, name
    table = so.contract()
    assert table["hj_zipf_next_dev"][0] == "waits" and table["hj_join_dev"][0] == "reads back"
    assert "HJ_ALGO_HTM" in table["hj_build_dev"][1]         # the exception the htm sequence skips the assertion for
    for name, (cls, _note) in table.items():
        if name.endswith("_info") and "layout" not in name and name not in ("hj_prj_workspace_info", "hj_prj_fragment_info"):
            assert cls == "waits", (name, cls)


def test_the_parser_refuses_a_broken_table(tmp_path):
    good = open(os.path.join(so.ROOT, "INTEGRATION.md")).read()
    head = good[:good.index("Stream contract")]
    cases = {"no table": head + "Stream contract\n\nnothing here\n",
             "twice": head + "Stream contract\n\n| entry point | class |\n|---|---|\n| `hj_run` | waits |\n| `hj_run` | waits |\n",
             "two names": head + "Stream contract\n\n| entry point | class |\n|---|---|\n| `hj_run`, `hj_reserve` | waits |\n"}
    for name, text in cases.items():
        p = tmp_path / "doc.md"
        p.write_text(text)
        with pytest.raises(ValueError):
            so.contract(str(p))
    p = tmp_path / "doc.md"
    p.write_text(head + "Stream contract\n\n| entry point | class | notes |\n|---|---|---|\n| `hj_run` | waits | x |\n\n| `hj_reserve` | waits | |\n")
    assert so.contract(str(p)) == {"hj_run": ("waits", "x")}    # the table is one block of lines
