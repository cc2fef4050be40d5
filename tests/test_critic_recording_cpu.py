"""CPU: learning._SlotLayout -- the ONE place that knows how a slot of a recorded critic update's input ring is laid out
([B int64 indices | n_pad int32 ids | int32 log slot, int32 pad | int64 draw], rounded to 16 bytes) -- against a verbatim
restatement of the arithmetic it replaced (commit d604b36: the first-pass block of _critic_update_graphed and
_FastStep.__init__) and against every clause of ssac_step_create's geometry check (csrc/ssac_elementwise.hip), restated
here.  No GPU, no kernel."""
import itertools

import numpy as np
import pytest

GRID = list(itertools.product((1, 2, 3, 96, 128, 512, 4096), (1, 2, 3, 5, 10, 16)))


@pytest.mark.parametrize("B,n_sub", GRID)
def test_the_layout_is_the_parents_arithmetic(B, n_sub):
    from super_sac_amd import learning as L
    lay = L._SlotLayout(B, n_sub)
    # ---- the parent's formulas
    n_pad = (n_sub + 1) // 2 * 2
    nbytes = (8 * B + 4 * n_pad + 16 + 15) // 16 * 16
    assert (lay.B, lay.n_sub) == (B, n_sub)
    assert lay.n_pad == n_pad
    assert lay.nbytes == nbytes
    assert lay.ids_off == 8 * B                          # ssac_step_create's ids_off, the views' first cut
    assert lay.logslot_off == 8 * B + 4 * n_pad          # ssac_step_create's logslot_off
    assert lay.draw_off == 8 * B + 4 * n_pad + 8         # ssac_step_create's draw_off, ctx.tick_ptr - inbuf
    assert lay.slot_words == nbytes // 4                 # _lib.Feed: slot size in 4-byte words
    assert lay.logslot_word == (8 * B + 4 * n_pad) // 4  # _lib.Feed: word of the log slot
    with pytest.raises(AttributeError):
        lay.nbytes = 0


@pytest.mark.parametrize("B,n_sub", GRID)
def test_the_layout_passes_the_c_steps_geometry_check(B, n_sub):
    from super_sac_amd import learning as L
    lay = L._SlotLayout(B, n_sub)
    n_slots, event_every = L.FEED_SLOTS, L.EVENT_EVERY
    slot_bytes, n_rows, n_ids = lay.nbytes, lay.B, lay.n_sub
    ids_off, logslot_off, draw_off = lay.ids_off, lay.logslot_off, lay.draw_off
    assert slot_bytes % 16 == 0
    assert 8 * n_rows <= ids_off
    assert ids_off + 4 * n_ids <= logslot_off
    assert logslot_off + 4 <= slot_bytes
    assert draw_off % 8 == 0
    assert draw_off + 8 <= slot_bytes
    assert n_slots % event_every == 0


@pytest.mark.parametrize("B,n_sub", GRID)
def test_the_staging_views_have_their_shapes_and_do_not_overlap(B, n_sub):
    from super_sac_amd import learning as L
    lay = L._SlotLayout(B, n_sub)
    slots = L.FEED_SLOTS
    stage = np.zeros((slots, lay.nbytes), np.uint8)
    np_idx, np_i32, np_draw = lay.host_views(stage)
    assert (np_idx.dtype, np_i32.dtype, np_draw.dtype) == (np.int64, np.int32, np.int64)
    assert np_idx.shape == (slots, B) and np_i32.shape == (slots, lay.n_pad + 2) and np_draw.shape == (slots, 1)
    for v in (np_idx, np_i32, np_draw):
        assert np.shares_memory(v, stage)
    # distinct patterns, every byte of every view set, written in one order and read back after all are in
    row = np.arange(slots, dtype=np.int64)[:, None]
    pat_idx = 0x0101010101010101 * (1 + row % 100) + np.arange(B, dtype=np.int64)[None, :]
    pat_i32 = (-0x01010101 * (1 + row % 100) - np.arange(lay.n_pad + 2)[None, :]).astype(np.int32)
    pat_draw = -0x0202020202020202 * (1 + row % 50)
    np_idx[:], np_i32[:], np_draw[:] = pat_idx, pat_i32, pat_draw
    assert np.array_equal(np_idx, pat_idx) and np.array_equal(np_i32, pat_i32) and np.array_equal(np_draw, pat_draw)
    np_draw[:], np_i32[:], np_idx[:] = pat_draw, pat_i32, pat_idx   # (and in the other order)
    assert np.array_equal(np_idx, pat_idx) and np.array_equal(np_i32, pat_i32) and np.array_equal(np_draw, pat_draw)
    # the views sit where the C step writes: indices at 0, ids at ids_off, log slot at logslot_off, draw at draw_off
    raw = stage[5]
    assert np.array_equal(raw[:8 * B].view(np.int64), pat_idx[5])
    assert np.array_equal(raw[lay.ids_off:lay.ids_off + 4 * n_sub].view(np.int32), pat_i32[5, :n_sub])
    assert raw[lay.logslot_off:lay.logslot_off + 4].view(np.int32)[0] == pat_i32[5, lay.n_pad]
    assert raw[lay.draw_off:lay.draw_off + 8].view(np.int64)[0] == pat_draw[5, 0]
    # ... and together they leave only the rounding bytes behind the draw number untouched
    stage[:] = 0
    np_idx[:], np_i32[:], np_draw[:] = -1, -1, -1
    assert int((stage == 0xFF).sum()) == slots * (lay.draw_off + 8) and not stage[:, lay.draw_off + 8:].any()
