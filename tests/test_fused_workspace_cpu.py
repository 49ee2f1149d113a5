"""The workspace of the fused 2-D / 3-D sweep (core.fused_layout, core.FusedWorkspace) without a GPU and without the
HIP library: the layout against the sums it replaced, written out once here from _native's constants, and the named
views of a workspace built on the CPU against that layout."""
import itertools

import pytest
import torch

from flooder_amd import _native, core

QW, CQ, FC, FH = _native.QUEUE_WORDS, _native.CELL_QUEUE_WORDS, _native.FINISH_CTL_WORDS, _native.FLAG_HIST_WORDS
CASES = [(S, n_slots, wit, owner)
         for S, per in ((1, 7), (1, 14), (5, 7), (5, 14), (5, 15), (300, 7), (300, 15))
         for n_slots in (S * per,) for wit, owner in itertools.product((False, True), repeat=2)]


def test_control_block_words_have_not_moved():
    assert (core.CTL_FLAG_COUNT, core.CTL_DEFER, core.CTL_HIST) == (1, 12, 48)
    assert FH % 2 == 0 and FC % 2 == 0 and CQ % 2 == 0 and QW % 2 == 0   # `top` (uint64) starts on an even word
    assert core.CTL_DEFER + _native.DEFER_CTL_WORDS <= core.CTL_HIST   # defer_ctl ends before the histogram


@pytest.mark.parametrize("S,n_slots,wit,owner", CASES)
def test_layout_is_the_sums_it_replaced(S, n_slots, wit, owner):
    regions, n_words = core.fused_layout(S, n_slots, wit, owner)
    # the arithmetic of _sweep_dimension_cell before fused_layout, transcribed
    CTL_HIST = core.CTL_HIST
    n_zeroed = (1 if wit else 0) * QW + CQ + FC + 2 * S + CTL_HIST + FH + n_slots
    n_plain = n_zeroed
    if owner:
        n_zeroed += (n_zeroed & 1) + 3 * n_slots
    front = QW if wit else 0
    expect = {"cell_queue": (front, CQ), "finish_ctl": (front + CQ, FC), "top": (front + CQ + FC, 2 * S),
              "ctl": (front + CQ + FC + 2 * S, CTL_HIST + FH), "face_bits": (front + CQ + FC + 2 * S + CTL_HIST + FH, n_slots)}
    if wit:
        expect["wit_queue"] = (0, QW)
    if owner:
        expect["face_owner"] = (n_plain + (n_plain & 1), 2 * n_slots)
        expect["result"] = (n_zeroed - n_slots, n_slots)
    assert n_words == n_zeroed and regions == expect
    # pairwise disjoint, in order, and all of [0, n_words) but the one pad word in front of the owner words
    spans = sorted(regions.values())
    assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] == n_words
    gaps = [(a + n, b) for (a, n), (b, _) in zip(spans, spans[1:]) if a + n != b]
    pad = [(n_plain, n_plain + 1)] if owner and n_plain & 1 else []
    assert gaps == pad
    assert regions["top"][0] % 2 == 0
    if owner:
        assert regions["face_owner"][0] % 2 == 0
        assert regions["result"] == (n_words - n_slots, n_slots)
        assert (n_slots & 1) == (n_plain & 1)   # an odd number of slots is what needs the pad word


def test_both_parities_of_the_pad_word_are_among_the_cases():
    pads = {core.fused_layout(S, n, wit, True)[0]["face_owner"][0] - sum(core.fused_layout(S, n, wit, False)[0]["face_bits"])
            for S, n, wit, owner in CASES if owner}
    assert pads == {0, 1}


def words_from(arena, view):
    assert view.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr()
    return (view.data_ptr() - arena.data_ptr()) // 4


@pytest.mark.parametrize("wit,owner", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("S,R,F,n_slots", [(5, 286, 15, None), (5, 286, 15, 33), (1, 64, 7, 7), (300, 257, 7, None)])
def test_workspace_views_alias_the_arena_at_the_layout_offsets(S, R, F, n_slots, wit, owner):
    ws = core.FusedWorkspace(S, R, F, n_slots, torch.device("cpu"), wit, owner)
    slots = S * F if n_slots is None else n_slots
    regions, n_words = core.fused_layout(S, slots, wit, owner)
    assert ws.n_words == n_words and ws.arena.shape == (n_words,) and ws.arena.dtype == torch.int32
    for name in ("wit_queue", "cell_queue", "finish_ctl", "top", "ctl", "face_bits", "face_owner", "result"):
        view = getattr(ws, name)
        if name not in regions:
            assert view is None, name
            continue
        first, words = regions[name]
        assert words_from(ws.arena, view) == first, name
        assert view.numel() * view.element_size() == 4 * words and view.is_contiguous(), name
        assert view.storage_offset() * view.element_size() == 4 * first, name
    assert ws.top.dtype == torch.int64 and ws.top.shape == (S,)
    assert ws.face_bits.dtype == torch.int32 and ws.face_bits.shape == (slots,)
    if owner:
        assert ws.result.dtype == torch.float32 and ws.result.shape == (slots,)
        assert words_from(ws.arena, ws.result) == n_words - slots
    ctl, fctl = regions["ctl"][0], regions["finish_ctl"][0]
    assert words_from(ws.arena, ws.flag_count) == ctl + core.CTL_FLAG_COUNT
    assert words_from(ws.arena, ws.defer_ctl) == ctl + core.CTL_DEFER
    assert words_from(ws.arena, ws.flag_hist) == ctl + core.CTL_HIST and ws.flag_hist.numel() == FH
    assert words_from(ws.arena, ws.top_count) == fctl + _native.FINISH_CTL_TOP_COUNT
    # the scratch: shapes and dtypes of the allocations _sweep_dimension_cell made itself
    tiles, chunks = (R + 63) // 64, (R + 255) // 256
    expect = {"planes": ((24 * S,), torch.float32), "hard": ((4 * core.FINISH_HARD_CAP,), torch.int64),
              "top_list": ((S,), torch.int32), "d2": ((S, R), torch.int32), "flags": ((3, S * tiles), torch.int32),
              "defer_list": ((5 * S * chunks,), torch.int32), "defer_c": ((5 * S * chunks,), torch.float32),
              "split": ((2, S), torch.int32), "wgt": ((S,), torch.float32)}
    for name, (shape, dtype) in expect.items():
        t = getattr(ws, name)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
        assert t.untyped_storage().data_ptr() != ws.arena.untyped_storage().data_ptr(), name


def test_arena_is_zeroed_where_no_prepare_launch_clears_it(monkeypatch):
    monkeypatch.setattr(core, "SWEEP_PREPARE_FUSED", False)
    ws = core.FusedWorkspace(5, 286, 15, None, torch.device("cpu"), True, False)
    assert int(ws.arena.abs().max()) == 0
    monkeypatch.setattr(core, "CELL_SUPER", False)
    ws = core.FusedWorkspace(5, 286, 15, None, torch.device("cpu"), False, False)
    assert int(ws.arena.abs().max()) == 0
    assert ws.defer_list is None and ws.defer_c is None and ws.split is None and ws.wgt is None
    assert not {"defer_ctl", "light_list", "heavy_list"} & set(ws.block_fields())


def test_a_callers_plane_buffer_is_kept():
    buf = torch.empty(8 + 24 * 5 + 8, dtype=torch.float32)
    planes = buf[8:8 + 24 * 5]
    ws = core.FusedWorkspace(5, 286, 15, None, torch.device("cpu"), True, False, planes=planes)
    assert ws.planes.data_ptr() == planes.data_ptr() and ws.block_fields()["plane_scratch"].data_ptr() == planes.data_ptr()


def test_block_fields_are_fields_of_the_parameter_block():
    known = dict(_native.FusedSweep._fields_)
    ws = core.FusedWorkspace(5, 286, 15, 33, torch.device("cpu"), True, True)
    fields = ws.block_fields()
    assert set(fields) <= set(known)
    # every buffer pointer the default path (witness sweep, probe, runs of four, ownership) hands to the library
    pointers = {"face_bits": ws.face_bits, "d2_scratch": ws.d2, "flag_list": ws.flags[0], "flag_count": ws.flag_count,
                "flag_key": ws.flags[1], "flag_hist": ws.flag_hist, "flag_sorted": ws.flags[2], "top": ws.top,
                "top_list": ws.top_list, "top_count": ws.top_count, "simplex_weight": ws.wgt, "plane_scratch": ws.planes,
                "wit_queue": ws.wit_queue, "wit_item_list": ws.split[0], "cell_queue": ws.cell_queue,
                "defer_list": ws.defer_list, "defer_c": ws.defer_c, "defer_ctl": ws.defer_ctl, "light_list": ws.split[0],
                "heavy_list": ws.split[1], "finish_ctl": ws.finish_ctl, "hard_scratch": ws.hard, "face_owner": ws.face_owner}
    assert set(pointers) | {"hard_cap"} == set(fields) and fields["hard_cap"] == core.FINISH_HARD_CAP
    for name, t in pointers.items():
        assert known[name] is _native.c_void_p and fields[name].data_ptr() == t.data_ptr(), name
    # ... and the block takes them by name (tensors become their addresses)
    blk = _native.FusedSweep(**fields)
    assert blk.flag_hist == ws.flag_hist.data_ptr() and blk.face_owner == ws.face_owner.data_ptr()
    # without the witness sweep and ownership their fields stay NULL
    plain = core.FusedWorkspace(5, 286, 15, None, torch.device("cpu"), False, False).block_fields()
    assert set(fields) - set(plain) == {"wit_queue", "wit_item_list", "face_owner"}
