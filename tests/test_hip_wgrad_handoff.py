"""GPU: the hand-off behind the K loop of the fixed-shape weight-gradient tiles (wgrad_fixed_kernel, csrc/ssac_gemm.hip).

Behind its last MFMA a tile of the fixed form parks its K-groups' partial tiles in the staging buffer that does not hold the
last chunk -- buffer 0 for an even number of K iterations, buffer 1 for an odd one -- with no barrier in front, sums them behind
ONE barrier, issues its optimizer stores, and only then reduces the gradient-norm partial (LDS words of its own, one barrier)
and draws the arrival ticket of the folded logs.  No sum changes its order, so the general kernel's bytes are the reference.

Harness, inputs, float64 references and bounds are those of wgrad_launch.py (zero Adam moments for float64: see there).

Rows.  test_hip_wgrad_fixed.py runs 256 and 384 rows, two and three iterations per K-group.  Here: 512 and 640 rows, four and
five -- one even and one odd count with more than one trip through the loop's own double buffering behind the first.

Gradient-norm slots.  A 64 x 64 tile writes the first of the four 32 x 32 slots it covers and zeroes the others; per slot the
float64 sum of squares of the float64 gradient (exact on grid inputs) is the reference.  A slot is a float32 sum of products
over a fixed tree: the square (1 rounding), at most 4 additions in the thread (its 4 elements, the bias gradient's square in
the fc1 tiles), 6 levels of the wave's xor tree, 4 levels over the 16 wave partials: 15 roundings on any path from an
element to the slot, all terms >= 0, so the relative error is at most 15 * 2^-24; SLOT_RTOL is 16 * 2^-24.  A reduction that
reads the wave partials before they are complete misses whole waves' sums (1/16 of a tile each), and a ticket drawn before the
slot stores have drained shows in the folded gradient norm (_check_f64) and in the log block's bytes.
"""
import numpy as np
import pytest

from wgrad_launch import ADAM, FixedLaunch, _case, _check_f64, _inputs, _same_bytes, switches_restored

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture(autouse=True)
def _switches_restored(ssa):
    with switches_restored(ssa):
        yield


SLOT_RTOL = 16 * 2.0 ** -24
# (dz2u rebuilt, late word, logs): every launch writes parameters, both moments, the target, the slots and the loss partials
MODES = [(False, None, "none"), (True, 0.25, "folded"), (False, None, "deferred")]


@pytest.mark.parametrize("n", [512, 640])
def test_even_and_odd_iteration_counts_beyond_three(ssa, n):
    """512 / 640 rows, N 1, in_dim 23 (iters 4 / 5): fixed against general as bytes over everything the launch writes, the
    fixed launch against float64 with zero moments."""
    case = _case(n, nets=1, in_dim=23, dz2="null")
    inp, ref = _inputs(case)
    for null, late, logs in MODES:
        L = FixedLaunch(ssa, case, inp, dict(ADAM, id=case["id"]))
        what = f"{case['id']} [dz2u {'rebuilt' if null else 'stored'}, late {late}, logs {logs}]"
        a = L.run_fold(True, dz2_null=null, late=late, logs=logs)
        b = L.run_fold(False, dz2_null=null, late=late, logs=logs)
        assert a["taken"] == 1 and b["taken"] == 0, f"{what}: took {a['taken']} / {b['taken']}"
        _same_bytes(a, b, what)
        _check_f64(L, a, ref, what, late=late, logs=logs)


def _slot_reference(case, ref, slot, layer):
    """float64 sums of squares per 32 x 32 slot of a layer's gradient as 64 x 64 tiles leave them: the tile's sum (with its
    rows' bias gradient where the tile owns it: fc1) in the slot of its first block, zero in the siblings"""
    w = ref["w1" if layer == 0 else "w2"][0][slot]
    rows, cols = w.shape
    gy, gx = (rows + 31) // 32, (cols + 31) // 32
    want = np.zeros((gy, gx))
    for by in range((rows + 63) // 64):
        for bx in range((cols + 63) // 64):
            t = w[64 * by:64 * by + 64, 64 * bx:64 * bx + 64]
            want[2 * by, 2 * bx] = (t * t).sum()
            if layer == 0 and bx == 0:   # (fc2's bias gradient belongs to the head workgroups)
                b = ref["b1"][0][slot][64 * by:64 * by + 64]
                want[2 * by, 2 * bx] += (b * b).sum()
    return want.reshape(-1)


@pytest.mark.parametrize("layer,name", [(1, "fc2"), (0, "fc1")])
def test_gradient_norm_slots_per_slot_with_the_ticket_drawn(ssa, layer, name):
    """256 rows / N 2, logs folded (the arrival ticket is drawn): every slot of the layer against float64, the folded log block
    and everything else as the general kernel's bytes."""
    case = _case(256, nets=2, in_dim=23, dz2="null")
    inp, ref = _inputs(case)
    L = FixedLaunch(ssa, case, inp, dict(ADAM, id=case["id"]))
    a, b = L.run_fold(True, logs="folded"), L.run_fold(False, logs="folded")
    assert a["taken"] == 1 and b["taken"] == 0
    rows = a["sumsq"][:L.ns * L.ss_stride].reshape(L.ns, L.ss_stride).astype(np.float64)
    for slot in range(L.ns):
        have = rows[slot, L.ss_off[layer]:L.ss_off[layer] + L.tiles[layer]]
        want = _slot_reference(case, ref, slot, layer)
        assert have.shape == want.shape
        assert float(want.max()) > 0 and int((want > 0).sum()) == (16 if layer == 1 else 4), f"{name}: the reference has no weight"
        bad = np.abs(have - want) > SLOT_RTOL * want
        assert not bad.any(), f"{name}, net {slot}: slots {np.nonzero(bad)[0].tolist()}: {have[bad].tolist()} vs {want[bad].tolist()}"
    assert a["logs"].tobytes() == b["logs"].tobytes(), f"{name}: the folded log block differs from the general kernel's"
    _same_bytes(a, b, name)
    _check_f64(L, a, ref, name, logs="folded")
