"""No GPU: the surface of the ragged beam search (samples whose encoder memories have different lengths in one step loop) --
the C header declares the entry points and _lib binds them with the same number of arguments; the table arithmetic (the
engine's own d2t_ragged_beam_tables, a host-only function, and its Python restatement) and the packing of the memories give
hand-checked values."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from doc2tex_amd import Model, _lib
from doc2tex_amd.engine import Engine, pack_memories, ragged_beam_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "d2t.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, f"include/d2t.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["d2t_decode_beam_batch_ragged", "d2t_decode_supports_ragged_beam", "d2t_ragged_beam_tables",
                                  "d2t_op_decoder_row_ragged_beam"])
def test_header_declares_and_lib_binds_with_matching_arity(name):
    args = _declaration(name)
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == len(args), (name, args)
    assert hasattr(_lib.load(), name), f"libd2t.so does not export {name}"


def test_ragged_entry_takes_packed_rows_and_host_lengths():
    args = _declaration("d2t_decode_beam_batch_ragged")
    assert args[1].startswith("const float*") and args[2] == "int32_t N" and args[3] == "const int32_t* T"
    uniform = _declaration("d2t_decode_beam_batch")
    assert len(uniform) == 9 and uniform[3] == "int32_t T"  # the uniform entry point is unchanged
    assert [a.split()[-1] for a in args[4:]] == [a.split()[-1] for a in uniform[4:]]  # the same outputs
    op = _declaration("d2t_op_decoder_row_ragged_beam")
    assert "const int32_t* row_map" in op and "const int32_t* anc" in op and "int32_t samples" in op
    assert len(_declaration("d2t_op_decoder_row_ragged")) == 24 and len(_declaration("d2t_op_decoder_row")) == 30


def _engine_tables(lengths):
    lib = _lib.load()
    n = len(lengths)
    T = (C.c_int32 * max(n, 1))(*lengths)
    row0, length = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    total = lib.d2t_ragged_beam_tables(n, T, row0, length)
    assert lib.d2t_ragged_beam_tables(n, T, None, None) == total  # (either output may be left out)
    return {"row0": list(row0)[:n], "len": list(length)[:n], "mem_rows": int(total)}


def test_tables_of_hand_written_length_lists():
    # per SAMPLE: less than a tile, not a multiple of 16, more than 64 tiles, one key
    t = ragged_beam_tables([7, 1100, 261, 16, 33, 1])
    assert t["row0"] == [0, 7, 1107, 1368, 1384, 1417]
    assert t["len"] == [7, 1100, 261, 16, 33, 1] and t["mem_rows"] == 1418
    assert ragged_beam_tables([1]) == {"row0": [0], "len": [1], "mem_rows": 1}
    u = ragged_beam_tables([406] * 5)  # equal lengths: the uniform [N][T][d] layout
    assert u["row0"] == [i * 406 for i in range(5)] and u["mem_rows"] == 5 * 406
    # the slices tile the packed buffer without gaps or overlap, at the largest call the entry point takes
    t = ragged_beam_tables([4096] * 1024)
    ends = [a + n for a, n in zip(t["row0"], t["len"])]
    assert t["row0"] == [0] + ends[:-1] and ends[-1] == t["mem_rows"] == 4096 * 1024 < 2 ** 31


@pytest.mark.parametrize("lengths", [[7, 1100, 261, 16, 33, 1], [1], [406, 260, 148], [5] * 9, [4096] * 1024, []])
def test_the_engines_own_table_arithmetic_agrees(lengths):
    assert _engine_tables(lengths) == ragged_beam_tables(lengths)


@pytest.mark.parametrize("lengths", [[0], [4, -1], [3, 0, 3]])
def test_tables_refuse_empty_memories(lengths):
    with pytest.raises(ValueError):
        ragged_beam_tables(lengths)


def test_packing_keeps_input_order_and_repeats_a_tensors_length_per_sample():
    g = torch.Generator().manual_seed(1)
    mems = [torch.randn(2, 5, 8, generator=g), torch.randn(1, 19, 8, generator=g), torch.randn(3, 16, 8, generator=g)]
    packed, lengths = pack_memories(mems)
    assert lengths == [5, 5, 19, 16, 16, 16] and packed.shape == (2 * 5 + 19 + 3 * 16, 8) and packed.is_contiguous()
    t = ragged_beam_tables(lengths)
    flat = [m[j] for m in mems for j in range(m.shape[0])]
    for i, want in enumerate(flat):  # sample i's slice of the packed rows is its memory, bit for bit
        assert torch.equal(packed[t["row0"][i]: t["row0"][i] + t["len"][i]], want)
    one, l1 = pack_memories([mems[1]])
    assert l1 == [19] and torch.equal(one, mems[1][0])
    with pytest.raises(ValueError):
        pack_memories([mems[0], torch.zeros(1, 4, 9)])  # another model width
    with pytest.raises(ValueError):
        pack_memories([torch.zeros(4, 8)])


def test_python_surface():
    assert callable(Engine.decode_beam_batch_ragged) and callable(Engine.supports_ragged_beam)
    assert list(inspect.signature(Engine.decode_beam_batch_ragged).parameters) == ["self", "packed", "lengths", "beam_size"]
    # the single-tensor call keeps its signature; the list form is served by a path of its own
    assert list(inspect.signature(Model.beam_search_batch).parameters) == ["self", "input", "beam_size", "return_attn"]
    assert callable(Model._beam_search_mixed)
