"""No GPU: the surface of ragged decode groups (batches of different row counts and memory lengths in one step loop) --
the C header declares the entry points and _lib binds them with the same number of arguments, the host helper that lays
out the per-row / per-batch tables gives hand-checked values, and Model carries the two switches with their defaults."""
import os
import re

import pytest

from doc2tex_amd import Model, _lib, synth
from doc2tex_amd.engine import ragged_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "d2t.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, f"include/d2t.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["d2t_decode_greedy_submit_ragged", "d2t_op_decoder_row_ragged", "d2t_decode_graph_count",
                                  "d2t_decode_supports_ragged"])
def test_header_declares_and_lib_binds_with_matching_arity(name):
    args = _declaration(name)
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == len(args), (name, args)
    assert hasattr(_lib.load(), name), f"libd2t.so does not export {name}"


def test_submit_ragged_takes_host_tables_and_packed_rows():
    args = _declaration("d2t_decode_greedy_submit_ragged")
    assert args[1].startswith("const float*") and args[2].startswith("int32_t n_batches")
    assert args[3] == "const int32_t* batch_rows" and args[4] == "const int32_t* batch_T"
    assert args[-1].startswith("int64_t*")  # the ticket
    # the uniform entry point is unchanged
    assert len(_declaration("d2t_decode_greedy_submit")) == 11 and len(_declaration("d2t_op_decoder_row")) == 30


def test_tables_of_hand_written_layouts():
    # three batches: 2 rows of 5 keys, ONE row of 19 keys (not a multiple of 16), 3 rows of 16 keys
    t = ragged_tables([(2, 5), (1, 19), (3, 16)])
    assert t["row0"] == [0, 5, 10, 29, 45, 61]
    assert t["len"] == [5, 5, 19, 16, 16, 16]
    assert t["row_batch"] == [0, 0, 1, 2, 2, 2]
    assert t["batch_rows"] == [2, 1, 3]
    assert t["rows"] == 6 and t["mem_rows"] == 2 * 5 + 19 + 3 * 16
    # a single one-row batch of one key
    assert ragged_tables([(1, 1)]) == {"row0": [0], "len": [1], "row_batch": [0], "batch_rows": [1], "rows": 1, "mem_rows": 1}
    # a uniform group is the special case row0[b] = b * T
    u = ragged_tables([(3, 261), (3, 261)])
    assert u["row0"] == [b * 261 for b in range(6)] and u["len"] == [261] * 6 and u["row_batch"] == [0, 0, 0, 1, 1, 1]
    # every row's slice lies inside the packed buffer and the slices do not overlap
    t = ragged_tables([(1, 406), (2, 148), (1, 7), (4, 1027)])
    ends = [a + n for a, n in zip(t["row0"], t["len"])]
    assert t["row0"] == [0] + ends[:-1] and ends[-1] == t["mem_rows"]


@pytest.mark.parametrize("layout", [[(0, 5)], [(2, 0)], [(1, 4), (-1, 4)]])
def test_tables_refuse_empty_batches(layout):
    with pytest.raises(ValueError):
        ragged_tables(layout)


def test_model_switches_and_their_defaults():
    m = Model(synth.make_config("T2", max_seq_len=8))
    assert m.decode_group_mixed is False
    assert m.decode_group_rows == 384
    assert m.decode_group == 1 and m.pipelined is False  # what runs today is what ran before
