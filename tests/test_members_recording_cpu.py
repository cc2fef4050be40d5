"""CPU: the host side of recorded ensemble critic updates (ensemble_size > 1, SUNRISE).  No GPU, no kernel.

* learning_utils.members_recordable -- the gate of learning.critic_update for agents with more than one member -- over
  every clause, against the rule restated here.
* learning._SlotLayout(E * B, E * n_sub): an E-member recording keeps the one-member layout and ssac_step_create's
  geometry; member i owns rows [i B, (i + 1) B) of the index block and ids [i n_sub, (i + 1) n_sub) of the id block, the
  aux word (the member whose gradient norm is logged) sits behind the log slot, and engine.CaptureCtx.set_member hands out
  exactly those blocks.
* learning._host_inputs -- the host draws of one recorded update, one member or several -- against a plain re-enactment
  of the reference's order on Python's `random` and torch's CPU generator: per member indices, then subset; behind the
  last subset the pick of learning.py:135 and a refresh's member pick; learning._close_update draws nothing more."""
import itertools
import random
import types

import numpy as np
import pytest
import torch


def _rule(launch_mode, E, identity, kind, per, refresh, dr3, process_call, bf16, sharded, weight_type, temp, max_members):
    """the issue's list, clause by clause"""
    if launch_mode != "list":
        return False
    if not 2 <= E <= max_members:
        return False
    if not identity:
        return False
    if kind not in ("stochastic", "deterministic", "discrete"):   # (not Beta)
        return False
    if per or refresh or dr3:
        return False
    if process_call:
        return False
    if bf16 or sharded:
        return False
    weights_off = weight_type is None or temp is None
    return weights_off or weight_type == "sunrise"


def test_members_recordable_truth_table():
    from super_sac_amd import learning_utils as lu
    M = lu.MAX_MEMBERS
    assert M == 8
    grid = itertools.product(("list", "graph"), (1, 2, 5, M, M + 1), (True, False),
                             ("stochastic", "deterministic", "discrete", "beta"), (False, True), (False, True),
                             (False, True), (False, True), (False, True), (False, True),
                             ((None, None), (None, 20.0), ("sunrise", None), ("sunrise", 20.0), ("softmax", 20.0),
                              ("softmax", None)))
    n_true = 0
    for mode, E, ident, kind, per, refresh, dr3, proc, bf16, sharded, (wt, temp) in grid:
        got = lu.members_recordable(mode, E, ident, kind, per, refresh, dr3, proc, bf16, sharded, wt, temp)
        assert got is _rule(mode, E, ident, kind, per, refresh, dr3, proc, bf16, sharded, wt, temp, M), \
            (mode, E, ident, kind, per, refresh, dr3, proc, bf16, sharded, wt, temp)
        n_true += got
    assert n_true == 3 * 3 * 5   # E in {2, 5, 8} x three heads x the five weight settings that are off or "sunrise"
    # the settings the existing recorded-update tests pin as eager stay out
    ok = dict(launch_mode="list", ensemble_size=2, identity_encoder=True, kind="stochastic", per=False,
              update_priorities=False, dr3=False, process_call=False, bf16=False, sharded=False, weight_type=None,
              weight_temp=None)
    assert lu.members_recordable(**ok)
    for change in (dict(process_call=True), dict(update_priorities=True), dict(launch_mode="graph"), dict(per=True),
                   dict(weight_type="softmax", weight_temp=1.0), dict(kind="beta"), dict(ensemble_size=1)):
        assert not lu.members_recordable(**dict(ok, **change)), change


@pytest.mark.parametrize("E,B,n_sub", [(2, 64, 2), (3, 64, 2), (5, 256, 2), (3, 5, 1), (8, 130, 3), (2, 96, 5)])
def test_member_major_views_of_the_slot(E, B, n_sub):
    from super_sac_amd import engine, learning as L
    lay = L._SlotLayout(E * B, E * n_sub)
    one = L._SlotLayout(B, n_sub)
    assert (lay.B, lay.n_sub) == (E * B, E * n_sub)
    # ssac_step_create's geometry check, unchanged
    assert lay.nbytes % 16 == 0 and 8 * lay.B <= lay.ids_off and lay.ids_off + 4 * lay.n_sub <= lay.logslot_off
    assert lay.logslot_off + 4 <= lay.nbytes and lay.draw_off % 8 == 0 and lay.draw_off + 8 <= lay.nbytes
    # ... and ssac_step_run_aux's: a free word behind the log slot, in front of the draw number
    assert lay.aux_off == lay.logslot_off + 4 and lay.aux_off + 4 <= lay.draw_off
    stage = np.zeros((L.FEED_SLOTS, lay.nbytes), np.uint8)
    np_idx, np_i32, np_draw = lay.host_views(stage)
    idx = np.arange(E * B, dtype=np.int64) * 3 + 1
    ids = [(7 * j) % 10 for j in range(E * n_sub)]
    np_idx[4] = idx
    np_i32[4, :E * n_sub] = ids
    np_i32[4, lay.n_pad], np_i32[4, lay.n_pad + 1], np_draw[4, 0] = 17, E - 1, 1234567
    raw = stage[4]
    for i in range(E):
        rows = raw[8 * i * B:8 * (i + 1) * B].view(np.int64)
        assert np.array_equal(rows, idx[i * B:(i + 1) * B]) and rows.size == one.B
        sub = raw[lay.ids_off + 4 * i * n_sub:lay.ids_off + 4 * (i + 1) * n_sub].view(np.int32)
        assert sub.tolist() == ids[i * n_sub:(i + 1) * n_sub]
    assert raw[lay.aux_off:lay.aux_off + 4].view(np.int32)[0] == E - 1
    assert raw[lay.logslot_off:lay.logslot_off + 4].view(np.int32)[0] == 17
    assert raw[lay.draw_off:lay.draw_off + 8].view(np.int64)[0] == 1234567
    # the capture hands every member its own block (the device views are stood in for by host tensors)
    inbuf = torch.from_numpy(raw.copy())
    idx_dev = inbuf[:lay.ids_off].view(torch.int64)
    ids_dev = inbuf[lay.ids_off:lay.logslot_off].view(torch.int32)[:E * n_sub]
    ctx = engine.CaptureCtx(torch.from_numpy(idx), idx_dev, ids, ids_dev, [], None)
    ctx.set_member(1)   # (members is None: a one-member capture keeps handing out everything)
    assert ctx.idx_dev is idx_dev and ctx.ids is ids and ctx.noise_offset == 0
    ctx.members = (E, B, n_sub)
    for i in (E - 1, 0, 1):
        ctx.set_member(i)
        assert ctx.idx_cpu.tolist() == idx[i * B:(i + 1) * B].tolist() == ctx.idx_dev.tolist()
        assert ctx.idx_dev.data_ptr() == idx_dev.data_ptr() + 8 * i * B
        assert ctx.ids == ids[i * n_sub:(i + 1) * n_sub] == ctx.ids_dev.tolist()
        assert ctx.ids_dev.data_ptr() == ids_dev.data_ptr() + 4 * i * n_sub
        assert ctx.noise_offset == i   # member i's noise: draw number (the slot's draw word) + i


class _Ring:
    def __init__(self):
        self.k = 0

    def advance(self):
        self.k += 1
        return self.k - 1


@pytest.mark.parametrize("E,B,N,n_sub,seed", [(3, 64, 2, 2, 17), (5, 256, 2, 2, 42), (2, 5, 10, 3, 3), (1, 64, 2, 2, 17),
                                              (1, 5, 10, 3, 3)])
def test_the_picks_place_in_the_python_random_stream(E, B, N, n_sub, seed):
    _the_picks_place(E, B, N, n_sub, seed, refresh=False)


def test_the_picks_place_behind_a_priority_refresh():
    _the_picks_place(1, 64, 2, 2, 42, refresh=True)


def _the_picks_place(E, B, N, n_sub, seed, refresh):
    from super_sac_amd import learning as L
    rows = 1000
    critics = [object() for _ in range(E)]
    agent = types.SimpleNamespace(critics=critics, ensemble_size=E)

    class _Buf:
        total_sample_calls = 0
        _per = types.SimpleNamespace(_raise_pending=lambda: None)

        def __len__(self):
            return rows
    buffer = _Buf()
    gs = types.SimpleNamespace(layout=L._SlotLayout(E * B, E * n_sub), n_members=E, fill=(([], []),) * E, n_critics=N,
                               log_ring=_Ring(), dev=None, pick=None, refresh=refresh, shard=None, k=0, deferred=None,
                               proc_dev=None, dicts=[{} for _ in range(E)], views=lambda slot_i: {"slot": slot_i})
    random.seed(seed); torch.manual_seed(seed)
    got = []
    for _ in range(4):
        idx_cpu, ids, slot_i, draw = L._host_inputs(gs, buffer, agent, False)
        assert L._aux_word(gs, {}) == (gs.pick if E > 1 else 0) and draw == 0
        state = (random.getstate(), torch.get_rng_state())
        logs, dicts = L._close_update(gs, agent, idx_cpu, ids, slot_i)
        # _close_update draws nothing: the picks were made before the update was issued
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
        for i, rd in enumerate(dicts):
            assert rd["priority_idxs"].tolist() == idx_cpu[i * B:(i + 1) * B].tolist()
            assert rd["_subset"] == ids[i * n_sub:(i + 1) * n_sub]
        got.append((idx_cpu.clone(), list(ids), gs.pick, slot_i))
    after = (random.getstate(), torch.get_rng_state())
    assert buffer.total_sample_calls == 4 * E and gs.k == 4
    # ---- the reference's order, re-enacted: per member torch.randint then random.sample; random.choice last, and behind
    # it the member pick of a priority refresh
    random.seed(seed); torch.manual_seed(seed)
    for u, (idx_cpu, ids, pick, slot_i) in enumerate(got):
        want_idx, want_ids = [], []
        for _ in range(E):
            want_idx.append(torch.randint(rows, (B,)))
            want_ids += random.sample(range(N), k=n_sub)
        want_pick = critics.index(random.choice(critics))
        if refresh:
            random.choice(range(1))
        assert torch.equal(idx_cpu, torch.cat(want_idx)) and ids == want_ids and pick == want_pick and slot_i == u
    assert random.getstate() == after[0] and torch.equal(torch.get_rng_state(), after[1])
