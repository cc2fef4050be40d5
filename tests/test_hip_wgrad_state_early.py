"""GPU: the fixed-shape weight-gradient tiles request their optimizer state one K iteration early (ssac_wgrad_state_early,
profiles/wgrad_state.md).

The switch moves loads and nothing else: the 16-byte request of p / m / v / target and of the control block, and the L2
touches in front of it, which the early form does not issue -- on the fc2 tiles and on fc1 tiles whose input width is a
multiple of 4.  (The same for the dword epilogue of an fc1 tile of any other width was built and measured; it gained nothing
and is not in the library, so such a tile loads as it did, beside fc2 tiles that take the early form.)  So every comparison
here is of BYTES, over everything the launch writes: the switch on against off, and both against the general kernel
(ssac_wgrad_fixed(0)).  Every test asserts through ssac_wgrad_state_early_taken() that the form it means to test actually ran.

The harness is test_hip_wgrad_fixed.FixedLaunch, whose arenas end in sentinel words, on SEEDED moments and targets: a request
aimed at another row, another arena or another net's block loads other numbers and shows in p, m, v or the target.

Shapes.  The early request stands in the K loop's last trip, so the trip count matters: 256 rows = two iterations per K-group
(the request sits in the loop's FIRST trip, right behind the first staging stores), 384 = three (the odd parking buffer), 512 =
four.  Widths 4 and 32 take the 16-byte epilogue on the fc1 tiles (the early request on an fc1 tile, with columns that do not
exist at width 4), 23 the dword one; every launch has fc2 tiles.  N = 2 puts a second net's block behind the first.
"""
import numpy as np
import pytest

import wgrad_cases as wc
from test_hip_store_through import _recorded_updates
from test_hip_wgrad_fixed import ADAM, FixedLaunch, _case, _inputs

pytestmark = pytest.mark.gpu
BIT16 = 1   # ssac_hip_test.h: bit 0 = the tiles on the 16-byte optimizer form
BYTES = ("params", "m", "v", "target", "sumsq", "partials", "td_out", "logs", "td_stats", "tick", "done")
# (dz2u rebuilt from h2, late word (None: static tau; 0.0: the bit clear, target neither loaded nor stored), target arena, logs)
MODES = [(True, None, 1, "folded"), (False, None, 0, "folded"), (True, 0.0, 1, "folded"), (True, wc.TAU, 1, "deferred")]


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture
def lib(ssa):
    """the library with every switch this file turns restored whatever a test does"""
    lib = ssa._lib.lib
    try:
        yield lib
    finally:
        lib.ssac_wgrad_state_early(-1)
        lib.ssac_store_through(-1)
        lib.ssac_fused_tile_rows(0)
        lib.ssac_wgrad_fixed(1)
        lib.ssac_wgrad_variant(0)


def _on_off_general(ssa, lib, L, want_bits, want_fixed, what, **opt):
    ssa._lib.check(lib.ssac_wgrad_state_early(-1))
    on = L.run_fold(True, **opt)
    took_on = lib.ssac_wgrad_state_early_taken()
    ssa._lib.check(lib.ssac_wgrad_state_early(0))
    off = L.run_fold(True, **opt)
    took_off = lib.ssac_wgrad_state_early_taken()
    ssa._lib.check(lib.ssac_wgrad_state_early(-1))
    gen = L.run_fold(False, **opt)
    took_gen = lib.ssac_wgrad_state_early_taken()
    assert on["taken"] == want_fixed and off["taken"] == want_fixed and gen["taken"] == 0, \
        f"{what}: fixed form {on['taken']} / {off['taken']} / {gen['taken']}"
    assert took_on == want_bits and took_off == 0 and took_gen == 0, f"{what}: took {took_on} / {took_off} / {took_gen}"
    assert set(on) == set(off) == set(gen)
    for k in BYTES:
        if k in on:
            assert on[k].tobytes() == off[k].tobytes(), f"{what}: {k} differs between the early and the late request"
            assert on[k].tobytes() == gen[k].tobytes(), f"{what}: {k} differs between the early request and the general kernel"
    for k in ("params", "m", "v", "target"):
        if k in on:   # (FixedLaunch hands the arenas back with the TAIL sentinel words that stand behind the last net)
            assert on[k].size == L.case["nets"] * L.stride + wc.TAIL
            assert bool((on[k][-wc.TAIL:] == wc.SENT).all()), f"{what}: {k} written past the arena"
    return on


@pytest.mark.parametrize("in_dim", [23, 4, 32])
@pytest.mark.parametrize("n,nets", [(256, 1), (384, 1), (512, 1), (256, 2), (384, 2), (512, 2)])
def test_early_state_request_gives_the_same_bytes(ssa, lib, n, nets, in_dim):
    """Two, three and four K iterations, N = 1 and 2, the 16-byte and the dword fc1 epilogue: Polyak on, no target arena,
    late-bound tau with the bit clear (the target is neither loaded nor stored), late-bound tau with deferred logs."""
    case = _case(n, nets=nets, in_dim=in_dim, dz2="null")
    inp, _ = _inputs(case)
    for null, late, target, logs in MODES:
        L = FixedLaunch(ssa, case, inp, dict(ADAM, target=target, seeded=1, id=case["id"]))
        what = f"{n} rows, {nets} nets, width {in_dim} [late {late}, target {target}, logs {logs}]"
        got = _on_off_general(ssa, lib, L, BIT16, 1, what, dz2_null=null, late=late, logs=logs)
        if late == 0.0:   # the bit clear: the target arena is what it was
            before = wc.adam_state(dict(ADAM, target=1, seeded=1, id=case["id"]), (nets, L.stride))[2]
            live = L.off[5] + case["out"]
            assert np.array_equal(got["target"][:nets * L.stride].reshape(nets, L.stride)[:, :live], before[:, :live]), what


@pytest.mark.parametrize("what,kw,ad", [
    ("weight decay", dict(), dict(ADAM, wd=1e-2)),
    ("per-row weights", dict(weight=1), dict(ADAM)),
])
def test_decay_and_weights_with_the_early_request(ssa, lib, what, kw, ad):
    """What travels in the control block (requested early with the state) and in the loss fold's arguments."""
    case = _case(256, nets=2, **kw)
    inp, _ = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ad, seeded=1, id=case["id"]))
    _on_off_general(ssa, lib, L, BIT16, 1, what, logs="folded")


@pytest.mark.parametrize("what,case,opt", [
    ("128 rows (two K-groups: the general kernel)", _case(128), {}),
    ("misaligned arena (the dword epilogue)", _case(256), dict(lead=1)),
])
def test_launches_outside_the_fixed_form_request_nothing_early(ssa, lib, what, case, opt):
    """A launch that does not take the fixed-shape form reports no bit and gives the same bytes."""
    inp, _ = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ADAM, target=1, seeded=1, id=case["id"]))
    _on_off_general(ssa, lib, L, 0, 0, what, logs="folded", **opt)


def test_recorded_updates_stay_on_the_same_bits(ssa, lib):
    """FEED_SLOTS + 3 recorded updates at B 256 / N 2 / width 23 with the switch on, then from the same seeds with it off: after
    every update the parameters, the targets, both moments, the TD targets and the logs as bytes.  The state that a tile
    requests early was written by the previous update's launch (through, on the fc2 tiles)."""
    ssa._lib.check(lib.ssac_wgrad_state_early(-1))
    on, _ = _recorded_updates(ssa, -1)
    took_on = lib.ssac_wgrad_state_early_taken()   # (a replayed update repeats the form of the launch that was recorded)
    ssa._lib.check(lib.ssac_wgrad_state_early(0))
    off, _ = _recorded_updates(ssa, -1)
    took_off = lib.ssac_wgrad_state_early_taken()
    assert took_on == BIT16 and took_off == 0, f"took {took_on} / {took_off}"
    assert len(on) == ssa.learning.FEED_SLOTS + 3 == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), f"update {k}: {name} differs between the early and the late request"
    assert np.isfinite(on[-1]["params"]).all() and float(np.abs(on[-1]["m"]).max()) > 0
    assert not np.array_equal(on[0]["params"], on[-1]["params"])
