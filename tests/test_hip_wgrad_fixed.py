"""GPU: the fixed-shape form of the merged weight-gradient launch (wgrad_fixed_kernel, csrc/ssac_gemm.hip) against the general
lean kernel it stands in for, and both against float64.

The fixed form leaves every floating-point operation and its order alone, so a launch with ssac_wgrad_fixed(1) and with (0) is
compared as BYTES over everything it writes: parameters, both moments, the target arena, the gradient-norm slots, the loss
partials, td_out and the logs (folded) or the TD statistics and the ring's tick (deferred).  Inputs, layouts, float64 references
and tolerances are those of wgrad_cases.py (the `lossfold` entry in Adam mode); the launch harness is wgrad_launch.FixedLaunch:
Launch with the log fold, the late-bound Polyak and a misaligned arena added.

Small launches take the 32 x 32 latency form by themselves: the 64 x 64 form is forced (ssac_wgrad_variant(1)).

Rows.  The fixed form is the lean kernel with FOUR K-groups, and the launcher gives a launch four K-groups from 8 chunks of 32
rows on (wgrad_merged: 2 below that), so 256 rows -- two iterations per K-group -- is the smallest launch that takes it and
384 the smallest with an odd iteration count.  At 128 rows (one chunk per K-group if there were four) the launch has two
K-groups and keeps the general kernel; the row ladder keeps that size and pins it as declined.  288 rows (nine chunks over four
groups) is the size at which the lean loader itself declines.

Weight decay, PopArt and per-row weights travel in the Adam control block and in the loss fold's arguments, which both forms
read alike: such launches TAKE the fixed form, with equal bits (test_decay_popart_and_weights_take_the_fixed_form).

What is the fixed form's alone (csrc/ssac_gemm.hip, ens_gemm_body): the lean hand-off behind the K loop
(test_hip_wgrad_handoff.py), the fc2 tiles' write-through optimizer stores, and the optimizer state requested one K iteration
early, from the K loop's last trip, with no L2 touches in front.  The last two move stores' cache policy and loads, nothing else,
so the general kernel's bytes are their reference too, on SEEDED moments and targets
(test_early_state_request_gives_the_same_bytes): a request or a store aimed at another row, another arena or another net's block
moves other numbers and shows in p, m, v or the target, or in the sentinel words behind the arenas.  The trip count matters to the early request: 256 rows = two iterations per K-group (the
request sits in the loop's FIRST trip, right behind the first staging stores), 384 = three (the odd parking buffer), 512 = four.
Widths 4 and 32 take the 16-byte epilogue on the fc1 tiles (the early request on an fc1 tile, with columns that do not exist at
width 4), 23 the dword one; every launch has fc2 tiles.  N = 2 puts a second net's block behind the first.

Float64 in Adam mode: zero moments and `_denom` (wgrad_launch.py).
"""
import numpy as np
import pytest

import wgrad_cases as wc
from wgrad_launch import (ADAM, FixedLaunch, Launch, _case, _check_f64, _check_grads, _check_lossfold, _inputs, _same_bytes,
                          recorded_updates, switches_restored)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture(autouse=True)
def _switches_restored(ssa):
    with switches_restored(ssa):
        yield


# (rows, nets, in_dim): the row ladder at the headline's width, the nets (per-class XCD mixing on only at N = 2: the class counts
# 16 N, 4 N, 4 N are multiples of 8 there), the input widths 4 / 23 (ragged last vector of the x rows) / 32 (a full block)
SHAPES = [(128, 1, 23), (256, 1, 23), (384, 1, 23), (256, 2, 23), (256, 3, 23), (256, 1, 4), (384, 2, 32)]
# (dz2u rebuilt, late word (None: static tau), target arena, logs, seeded moments: bytes only)
MODES = [(False, None, 1, "none", 0), (True, None, 1, "folded", 0), (False, wc.TAU, 1, "deferred", 0), (True, 0.0, 1, "folded", 0),
         (False, None, 0, "deferred", 0), (True, 0.125, 1, "none", 0), (True, wc.TAU, 1, "folded", 1)]
# the seeded-state comparisons: (dz2u rebuilt from h2, late word (None: static tau; 0.0: the bit clear, the target neither
# loaded nor stored), target arena, logs)
SEEDED_MODES = [(True, None, 1, "folded"), (False, None, 0, "folded"), (True, 0.0, 1, "folded"), (True, wc.TAU, 1, "deferred")]


def _fixed_equals_general(L, want_fixed, what, **opt):
    """one launch with the switch on and one with it off: the forms they report, everything they wrote as bytes, and the TAIL
    sentinel words that stand behind the last net of every arena; returns what the first wrote"""
    a, b = L.run_fold(True, **opt), L.run_fold(False, **opt)
    assert a["taken"] == want_fixed and b["taken"] == 0, f"{what}: took {a['taken']} / {b['taken']}"
    _same_bytes(a, b, what)
    for k in ("params", "m", "v", "target"):
        if k in a:
            assert a[k].size == L.case["nets"] * L.stride + wc.TAIL
            assert bool((a[k][-wc.TAIL:] == wc.SENT).all()), f"{what}: {k} written past the arena"
    return a


@pytest.mark.parametrize("n,nets,in_dim", SHAPES)
def test_fixed_form_gives_the_general_kernels_bits_and_the_float64_sums(ssa, n, nets, in_dim):
    """Every shape in every mode (dz2u stored / rebuilt from h2; static tau, a late word with a tau, a zero late word, no target;
    logs folded / deferred / none; seeded moments): fixed against general as bytes, the fixed launch against float64.  128 rows:
    declined."""
    case = _case(n, nets=nets, in_dim=in_dim, dz2="null")
    inp, ref = _inputs(case)
    for null, late, target, logs, seeded in MODES:
        ad = dict(ADAM, target=target, seeded=seeded, id=case["id"])
        L = FixedLaunch(ssa, case, inp, ad)
        what = f"{case['id']} [dz2u {'rebuilt' if null else 'stored'}, late {late}, target {target}, logs {logs}]"
        a = L.run_fold(True, dz2_null=null, late=late, logs=logs)
        b = L.run_fold(False, dz2_null=null, late=late, logs=logs)
        assert b["taken"] == 0 and a["taken"] == (0 if n < 256 else 1), f"{what}: took {a['taken']} / {b['taken']}"
        _same_bytes(a, b, what)
        if not seeded:
            _check_f64(L, a, ref, what, late=late, logs=logs)


@pytest.mark.parametrize("what,kw,ad", [
    ("weight decay", dict(), dict(ADAM, wd=1e-2)),
    ("PopArt", dict(popart=wc.POP_EXACT), dict(ADAM)),
    ("per-row weights", dict(weight=1), dict(ADAM)),
    ("given TD targets", dict(td="given"), dict(ADAM)),
])
def test_decay_popart_and_weights_take_the_fixed_form(ssa, what, kw, ad):
    """What reaches the launch through ssac_adam_ctl and LossFoldArgs is read by the same code in both forms: these launches take
    the fixed form, give the general kernel's bytes and match float64."""
    case = _case(256, nets=2, **kw)
    inp, ref = _inputs(case)
    logs = "folded"
    L = FixedLaunch(ssa, case, inp, dict(ad, id=case["id"]))
    a, b = L.run_fold(True, logs=logs), L.run_fold(False, logs=logs)
    assert a["taken"] == 1 and b["taken"] == 0, what
    _same_bytes(a, b, what)
    _check_f64(L, a, ref, what, logs=logs)


@pytest.mark.parametrize("what,kw,ad", [
    ("weight decay", dict(), dict(ADAM, wd=1e-2)),
    ("per-row weights", dict(weight=1), dict(ADAM)),
])
def test_decay_and_weights_with_the_early_request(ssa, what, kw, ad):
    """The same two launches on SEEDED moments, bytes only: what travels in the control block (requested with the state) and in
    the loss fold's arguments, with the sentinels behind the arenas."""
    case = _case(256, nets=2, **kw)
    inp, _ = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ad, seeded=1, id=case["id"]))
    _fixed_equals_general(L, 1, what, logs="folded")


@pytest.mark.parametrize("what,case,opt", [
    ("hidden 128", _case(256, H=128), {}),
    ("input of 33 columns", _case(256, in_dim=33), {}),
    ("160 rows", _case(160), {}),
    ("224 rows", _case(224), {}),
    ("288 rows", _case(288), {}),
    ("misaligned arena", _case(256), dict(lead=1)),
    ("gradient store", _case(256), dict(grads=True)),
])
def test_launches_outside_the_fixed_form_take_the_general_kernel(ssa, what, case, opt):
    """Each launch lacks one of the fixed form's conditions: it runs the general kernel with the switch on, and matches float64."""
    inp, ref = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ADAM, id=case["id"]))
    got = L.run_fold(True, **opt)
    assert got["taken"] == 0, what
    if opt.get("grads"):
        _check_grads(L, got, ref, "grid", what)
        _check_lossfold(L, got, "grid", what)
    else:
        _check_f64(L, got, ref, what)


@pytest.mark.parametrize("what,case", [
    ("net ids given", _case(256, nets=3, ids=(2, 0), entry="scaled")),
    ("two head outputs", _case(256, out=2, entry="all")),
])
def test_other_entry_points_never_take_the_fixed_form(ssa, what, case):
    """ssac_mlp_wgrad_all_lossfold takes neither a subset of the nets nor a head of two outputs: such launches come through
    ssac_mlp_wgrad_all_scaled / ssac_mlp_wgrad_all, in Adam mode at the fixed form's width, and keep the general kernel."""
    lib = ssa._lib.lib
    inp, ref = _inputs(case)
    ad = dict(ADAM, id=case["id"])
    L = Launch(ssa, case, inp, adam=ad)
    ssa._lib.check(lib.ssac_wgrad_fixed(1))
    got = L.run(variant=1)
    assert lib.ssac_wgrad_fixed_taken() == 0, what
    ctl = wc.adam_ctl(ad)
    old = dict(zip(("m", "v", "target"), wc.adam_state(ad, (case["nets"], L.stride))), p=inp["params"])
    got["p"] = got["params"]
    for slot in range(L.ns):
        for s in L.segs():
            g = ref[s][0][slot]
            o = {k: old[k][L.ids[slot], wc.seg_slices(case)[s]].reshape(g.shape) for k in ("m", "v", "p", "target")}
            r = wc.adam_ref(ctl, o["p"], g, o["m"], o["v"], o["target"])
            for k in ("m", "v", "p", "target"):
                have = L.seg_of(got[k], slot, s).astype(np.float64).reshape(g.shape)
                assert not (np.abs(have - r[k]) > wc.adam_tol(o[k], r[k])).any(), f"{what}: {k} of {s}, slot {slot}"


@pytest.mark.parametrize("setting", ["plain", "popart", "per-row weights"])
def test_recorded_update_ends_on_the_same_bits_with_either_form(ssa, setting):
    """Whole updates -- eager, recorded and replayed, Polyak every second -- with the switch on and off: final arenas, moments,
    targets and every update's logs equal as bytes.  B 256 / N 2: the smallest batch whose weight-gradient launch has four
    K-groups (module docstring).  PopArt needs the target Q in one part, which the engine forms at the benchmark's shape only."""
    kw = dict(pop=setting == "popart", weights=setting == "per-row weights")
    if setting == "popart":
        kw.update(B=512, N=10)
    kw = dict(dict(B=256, N=2, n_upd=6), **kw)
    (a,), taken_a = recorded_updates(ssa, fixed=True, **kw)
    (b,), taken_b = recorded_updates(ssa, fixed=False, **kw)
    print(setting, "weight-gradient launches took (switch on):", taken_a, "(off):", taken_b)
    assert all(t == 0 for t in taken_b)
    if setting == "plain":
        assert all(t == 1 for t in taken_a)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{setting}: {k} differs between the fixed and the general form"
    assert np.isfinite(a["params"]).all() and float(np.abs(a["m"]).max()) > 0


@pytest.mark.parametrize("in_dim", [23, 4, 32])
@pytest.mark.parametrize("n,nets", [(256, 1), (384, 1), (512, 1), (256, 2), (384, 2), (512, 2)])
def test_early_state_request_gives_the_same_bytes(ssa, n, nets, in_dim):
    """Seeded moments and targets; two, three and four K iterations, N = 1 and 2, the 16-byte and the dword fc1 epilogue (module
    docstring): Polyak on, no target arena, late-bound tau with the bit clear (the target is neither loaded nor stored),
    late-bound tau with deferred logs.  Fixed against general over BYTES, the sentinels behind the arenas.
    (The write-through stores' own comparison -- width 23, 256 / 384 rows, N 1 / 2, these modes -- was a strict subset of this
    one and is not repeated.)"""
    case = _case(n, nets=nets, in_dim=in_dim, dz2="null")
    inp, _ = _inputs(case)
    for null, late, target, logs in SEEDED_MODES:
        L = FixedLaunch(ssa, case, inp, dict(ADAM, target=target, seeded=1, id=case["id"]))
        what = f"{n} rows, {nets} nets, width {in_dim} [late {late}, target {target}, logs {logs}]"
        got = _fixed_equals_general(L, 1, what, dz2_null=null, late=late, logs=logs)
        if late == 0.0:   # the bit clear: the target arena is what it was
            before = wc.adam_state(dict(ADAM, target=1, seeded=1, id=case["id"]), (nets, L.stride))[2]
            live = L.off[5] + case["out"]
            assert np.array_equal(got["target"][:nets * L.stride].reshape(nets, L.stride)[:, :live], before[:, :live]), what


def test_seeded_launches_outside_the_fixed_form_ignore_the_switch(ssa):
    """128 rows (two K-groups) and a misaligned arena (the dword epilogue), seeded, with a target: with the switch on and off both
    launches report the general kernel and give equal bytes, the sentinels intact."""
    for what, case, opt in (("128 rows", _case(128), {}), ("misaligned arena", _case(256), dict(lead=1))):
        inp, _ = _inputs(case)
        L = FixedLaunch(ssa, case, inp, dict(ADAM, target=1, seeded=1, id=case["id"]))
        _fixed_equals_general(L, 0, what, logs="folded", **opt)


def test_recorded_updates_stay_on_the_same_bits(ssa):
    """FEED_SLOTS + 3 recorded updates (the input ring wraps) at B 256 / N 2 / width 23 with 32-row critic tiles, in the fixed
    form and from the same seeds in the general one: after EVERY update the parameters, the targets, both moments, the TD targets
    and the logs as bytes.  The state a tile requests early was written through by the previous update's launch: a reader that
    still found a stale line would show as a difference that grows from the update it first happens in."""
    kw = dict(B=256, N=2, pop=False, weights=False, n_upd=ssa.learning.FEED_SLOTS + 3, tile_rows=32, every_update=True)
    a, taken_a = recorded_updates(ssa, fixed=True, **kw)
    b, taken_b = recorded_updates(ssa, fixed=False, **kw)
    assert all(t == 1 for t in taken_a) and all(t == 0 for t in taken_b), f"took {taken_a} / {taken_b}"
    assert len(a) == ssa.learning.FEED_SLOTS + 3 == len(b) == len(taken_a) == len(taken_b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y) == {"params", "target", "m", "v", "td", "logs"}
        for name in x:
            assert x[name].tobytes() == y[name].tobytes(), f"update {k}: {name} differs between the fixed and the general form"
    assert np.isfinite(a[-1]["params"]).all() and float(np.abs(a[-1]["m"]).max()) > 0
    assert not np.array_equal(a[0]["params"], a[-1]["params"])
