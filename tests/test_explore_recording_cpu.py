"""CPU: the two host-side decisions behind recorded critic updates that carry an exploration process.

The slot's aux word: learning._SlotLayout.aux_off names the int32 pad behind the log slot, which carries the bits of the
process's scale (ssac_step_run_aux in C, _write_slot's np_i32[:, n_pad + 1] in Python) without moving any other field.
The recording predicate: learning_utils.explore_recordable against a restatement of the rule.  No GPU, no kernel."""
import itertools
import struct

import numpy as np
import pytest

from test_critic_recording_cpu import GRID


@pytest.mark.parametrize("B,n_sub", GRID)
def test_the_aux_word_is_the_pad_behind_the_log_slot(B, n_sub):
    from super_sac_amd import learning as L
    lay = L._SlotLayout(B, n_sub)
    assert lay.aux_off == lay.logslot_off + 4
    assert lay.aux_off + 4 <= lay.draw_off                           # ends where the draw number starts, at the latest
    assert lay.nbytes == (8 * B + 4 * lay.n_pad + 16 + 15) // 16 * 16   # the slot did not grow
    stage = np.zeros((L.FEED_SLOTS, lay.nbytes), np.uint8)
    np_idx, np_i32, np_draw = lay.host_views(stage)
    bits = struct.unpack("<i", struct.pack("<f", 0.3125))[0]
    np_i32[7, lay.n_pad + 1] = bits                                  # what _write_slot stores
    raw = stage[7]
    assert raw[lay.aux_off:lay.aux_off + 4].view(np.float32)[0] == np.float32(0.3125)
    assert int((stage != 0).sum()) == int((raw[lay.aux_off:lay.aux_off + 4] != 0).sum())   # nothing else was touched
    # ... and neither the log slot nor the draw number reaches into it
    stage[:] = 0
    np_i32[:, lay.n_pad] = -1
    np_draw[:] = -1
    np_idx[:] = -1
    np_i32[:, :n_sub] = -1
    assert not stage[:, lay.aux_off:lay.aux_off + 4].any()


def test_the_scale_bits_round_trip():
    """_aux_word hands ssac_step_run_aux / _write_slot an int32 whose bytes are the float's; the picked member for an
    ensemble; 0 for a recording with neither"""
    import types
    from super_sac_amd import learning as L
    for scale in (0.0, 1.0, 0.1, 0.7, 1e-3, 2.5):
        gs = types.SimpleNamespace(proc_dev=object(), n_members=1)
        bits = L._aux_word(gs, {"random_process": types.SimpleNamespace(current_scale=scale)})
        assert -2 ** 31 <= bits < 2 ** 31
        assert np.array([bits], np.int32).view(np.float32)[0] == np.float32(scale)
    assert L._aux_word(types.SimpleNamespace(proc_dev=None, n_members=1), {"random_process": None}) == 0
    assert L._aux_word(types.SimpleNamespace(proc_dev=None, n_members=3, pick=2), {"random_process": None}) == 2
    assert L._aux_word(types.SimpleNamespace(proc_dev=None, n_members=1, pick=0), {}) == 0


def _rule(kind, has_process, discrete, identity_encoder, E, per, sharded, launch_mode):
    """the issue's rule, restated: a process blocks the recording unless the update ignores it (discrete agents) or every
    one of the listed conditions holds"""
    if not has_process:
        return True
    if discrete:
        return True
    if launch_mode != "list":
        return False
    if kind not in ("stochastic", "deterministic"):
        return False
    if not identity_encoder or E != 1 or per or sharded:
        return False
    return True


def test_the_recording_predicate_over_the_grid():
    from super_sac_amd import learning_utils as lu
    n = n_true = 0
    for kind, has_process, encoder, E, per, shard, mode in itertools.product(
            ("stochastic", "deterministic", "beta", "discrete"), (False, True), ("identity", "pixel", "mlp"), (1, 2, 5),
            (False, True), (None, "critic", "member"), ("list", "graph")):
        discrete = kind == "discrete"
        got = lu.explore_recordable(kind, has_process, discrete, encoder == "identity", E, per, shard is not None, mode)
        assert got == _rule(kind, has_process, discrete, encoder == "identity", E, per, shard is not None, mode), \
            (kind, has_process, encoder, E, per, shard, mode)
        n += 1
        n_true += got
    assert n == 4 * 2 * 3 * 3 * 2 * 3 * 2
    # without a process and for discrete agents nothing is decided here; with one, exactly the two continuous heads on the
    # one supported configuration pass
    with_process_continuous = [k for k in ("stochastic", "deterministic", "beta")
                               if lu.explore_recordable(k, True, False, True, 1, False, False, "list")]
    assert with_process_continuous == ["stochastic", "deterministic"]
    assert 0 < n_true < n
