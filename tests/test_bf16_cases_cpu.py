"""CPU: the inputs and bounds of bf16_cases.py are fit for purpose -- no kernel runs here.
  * the fragment layout helpers invert each other and match the documented frag_off formula;
  * every grid case is exact: a float32 evaluation with the bf16 re-rounding emulated gives the float64 bits in two K orders;
  * exact-scale cases: c and c * dz are exact in float32; general cases: under 1 % of the terms are flagged and every unflagged
    term of the float32 emulation rounds to the reference's bf16 value;
  * losing any planted row moves every output element by at least 100 x its bound;
  * the measured constants (float32 emulation in the kernel's orders vs float64) are at or below the recorded ones;
  * the Adam bound tells the right operation order from a wrong one and covers a float32 evaluation of adam_elem."""
import numpy as np
import pytest

import bf16_cases as bc
from wgrad_cases import EPS24, F32, F64, SEGS, adam_ctl

def test_fragment_layout_round_trip_and_formula():
    g = np.random.RandomState(0)
    for rows, bp in ((32, 16), (96, 48), (64, 272)):
        m = bc.bf16_round(g.standard_normal((rows - 5, bp - 3)).astype(F32))
        buf = bc.to_frag(m, rows, bp, pad_bits=bc.PAD_ONE)
        back = bc.from_frag(buf, rows, bp)
        assert np.array_equal(bc.bf16_widen(back[:rows - 5, :bp - 3]), m)
        assert bool((back[:, bp - 3:] == bc.PAD_ONE).all()) and not back[rows - 5:, :bp - 3].any()
        steps = bp // 16
        for n, k in ((0, 0), (26, 12), (rows - 6, bp - 4), (33 % (rows - 5), 9)):
            off = (((n // 32) * steps + k // 16) * 64 + n % 32 + 32 * (k // 8 % 2)) * 8 + k % 8
            assert buf[off] == bc.bf16_bits(m[n, k])


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 3.0e-5, 0.0], F32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, 0.0], F32)
    got = bc.bf16_round(x)
    assert np.array_equal(got[:5], want[:5]) and got[6] == 0.0 and abs(got[5] - 3.0e-5) <= 2.0 ** -8 * 3.0e-5
    import torch
    z = np.random.RandomState(1).standard_normal(4096).astype(F32)
    assert np.array_equal(bc.bf16_round(z), torch.from_numpy(z).to(torch.bfloat16).to(torch.float32).numpy())


def test_case_list_covers_the_shapes_the_kernel_branches_on():
    cs = bc.GRAD_CASES
    for key, want in (("H", {32, 64, 96, 256}), ("in_dim", {1, 16, 17, 23, 64, 65, 100}), ("nets", {1, 3, 5}),
                      ("n", {1, 15, 16, 17, 100, 255, 256, 257, 272, 1000, 8192})):
        assert {c[key] for c in cs} == want, key
    assert len(cs) <= 28
    for h in (32, 96):   # every ragged hidden meets a ragged in_dim and a ragged row count
        assert any(c["H"] == h and c["in_dim"] % 16 and c["n"] % 16 for c in cs)
    grids = {bc.wgrad_tiles(c) * c["nets"] for c in cs}
    assert {3, 9, 15} <= grids and sum(1 for x in grids if x % 8) >= 8
    kinds = [k for c in cs for k in bc.kinds(c)]
    assert kinds.count("grid") >= 8 and any(c["n"] == 8192 and bc.kinds(c) == ("grid",) for c in cs)
    gen = [c for c in cs if "general" in bc.kinds(c)]
    assert {(c["popart"] is bc.POP_GENERAL, c["pop"]) for c in gen} >= {(True, 0), (True, 1), (False, 1)}
    assert {c["td"] for c in gen} == {"given", "lazy"} and {c["weight"] for c in gen} == {0, 1}
    for kind, cid in bc.PAD_CASES.items():
        assert kind in bc.kinds(bc._ALL[cid]) and bc._ALL[cid]["n"] % 16


@pytest.mark.parametrize("cid", bc.ids([c for c in bc.GRAD_CASES + bc.ADAM_CASES if "grid" in bc.kinds(c) or "wd" in c]))
def test_grid_cases_are_exact_in_float32_in_two_orders(cid):
    case = bc._ALL[cid]
    assert bc.grid_ok(case)
    if "wd" in case:
        inp = bc.make_inputs(case, "grid")
        ref = bc.reference(case, inp)
    else:
        _, inp, ref = bc.load(cid, "grid")
    assert ref["flag_share"] == 0.0
    for order in (bc.emul_steps, bc.emul_steps_rev):
        em = bc.emulate(case, inp, order)
        for s in SEGS:
            want = ref[s][0].astype(F32)
            assert np.array_equal(want.astype(F64), ref[s][0]), f"{cid}: {s} is not a float32 number"
            assert np.array_equal(em[s].reshape(want.shape), want), f"{cid}: {s} is not exact in float32 ({order.__name__})"


@pytest.mark.parametrize("cid", bc.ids([c for c in bc.GRAD_CASES if "exact" in bc.kinds(c)]))
def test_gauss_cases_margins_flags_and_measured_constants(cid):
    case = bc._ALL[cid]
    for kind in ("exact", "general"):
        _, inp, ref = bc.load(cid, kind)
        ls = ref["loss"]
        c32 = bc.loss_scale(case, inp, F32)["c"]
        if kind == "exact":
            assert np.array_equal(c32.astype(F64), ls["c"]), f"{cid}: the row scale is not exact in float32"
            for dz in (inp["DZ1"], inp["DZ2"]):
                p = ls["c"][..., None] * dz.astype(F64)
                assert np.array_equal(p.astype(F32).astype(F64), p), f"{cid}: c * dz is not exact in float32"
            assert ref["flag_share"] == 0.0
        else:
            assert bool((np.abs(c32.astype(F64) - ls["c"]) <= 0.5 * ls["u_c"]).all()), f"{cid}: u_c does not cover the float32 evaluation"
            assert ref["flag_share"] < 0.01, f"{cid}: {ref['flag_share']:.4f} of the terms are flagged"
            for dz in (inp["DZ1"], inp["DZ2"]):   # an unflagged term rounds to the reference's bf16 value
                _, s, fl, _ = bc.scaled(ls["c"], dz, ls["u_c"])
                s32 = bc.bf16_round((c32[..., None] * dz).astype(F32)).astype(F64)
                assert bool(((s32 == s) | fl).all()), f"{cid}: an unflagged term rounds differently in float32"
                assert bool((np.abs(s32 - s) <= bc.bf16_ulp(np.maximum(np.abs(s), np.abs(s32))) * 1.0000001).all())
        # planted rows
        terms = bc.planted_terms(case, inp, ref)
        em = bc.emulate(case, inp)
        for s in SEGS:
            g, S, extra = ref[s]
            bnd = bc.bound(kind, s, S, extra)
            margin = terms[s].reshape((-1,) + g.shape) / np.maximum(bnd, 1e-300)[None]
            assert float(margin.min()) >= 100.0, f"{cid} [{kind}]: losing a planted row moves an element of {s} by {float(margin.min()):.1f} bounds only"
            dev = (np.abs(em[s].reshape(g.shape).astype(F64) - g) - extra) / np.maximum(EPS24 * S, 1e-300)
            key = "C_WEIGHT" if s[0] == "w" else "C_BIAS"
            assert float(dev.max()) <= bc.MEASURED[kind][key], f"{cid} [{kind}]: {s} measures {float(dev.max()):.2f}, recorded {bc.MEASURED[kind][key]}"


def test_constants_follow_the_recorded_measurements():
    for kind in ("exact", "general"):
        for key in ("C_WEIGHT", "C_BIAS"):
            assert bc.C_GRAD[kind][key] == max(8.0, 4.0 * bc.MEASURED[kind][key])
    assert bc.C_Q == max(8.0, 4.0 * bc.MEASURED["C_Q"])


def _adam32(ctl, p, g, m, v):
    """adam_elem in float32 with IEEE square root and reciprocal"""
    f = lambda k: F32(ctl[k])
    one = F32(1.0)
    if ctl["wd"] != 0.0:
        g = g + f("wd") * p
    m = m + (one - f("beta1")) * (g - m)
    v = v * f("beta2") + (one - f("beta2")) * g * g
    den = np.sqrt(v) * (one / f("bc2_sqrt")) + f("eps")
    return dict(m=m, v=v, p=p - f("step_size") * (m * (one / den)))


@pytest.mark.parametrize("seeded,wd", [(0, 0.0), (1, 1e-2)])
def test_adam_bound_covers_float32_and_rejects_a_wrong_order(seeded, wd):
    g_ = np.random.RandomState(5)
    case = dict(seeded=seeded, wd=wd)
    ctl = adam_ctl(case)
    n = 20000
    p, g = g_.standard_normal(n).astype(F32), (g_.randint(-64, 65, n) * 0.25).astype(F32)
    m = (g_.standard_normal(n) * 0.5).astype(F32) if seeded else np.zeros(n, F32)
    v = g_.uniform(0.1, 2.0, n).astype(F32) if seeded else np.zeros(n, F32)
    ref = bc.adam_ref(ctl, p, g, m, v, None)
    got = _adam32(ctl, p, g, m, v)
    for k in ("m", "v", "p"):
        val, err = ref[k]
        assert bool((np.abs(got[k].astype(F64) - val) <= bc.adam_tol(val, err)).all()), k
        # the bound is a few ulp, not a tolerance that would swallow a wrong formula
        # (a parameter can land near zero, a first moment can cancel: the step and the moment's inputs are their scales)
        scale = np.abs(val) + {"p": float(ctl["step_size"]), "m": np.abs(m) + np.abs(g), "v": 0.0}[k]
        assert float((bc.adam_tol(val, err) / np.maximum(scale, 1e-30))[scale > 1e-3].max()) < 2e-5, k
    if wd:   # weight decay added AFTER the first moment: must be outside the bound somewhere
        wrong_m = m + (F32(1.0) - F32(ctl["beta1"])) * (g - m)
        assert bool((np.abs(wrong_m.astype(F64) - ref["m"][0]) > bc.adam_tol(*ref["m"])).any())
    # a step taken with 1 - beta2^t instead of its square root, or without the bias correction, is far outside
    val, err = ref["p"]
    no_bc = p.astype(F64) - float(ctl["step_size"]) * (ref["m"][0] / (np.sqrt(ref["v"][0]) + float(ctl["eps"])))
    moved = np.abs(val - p) > 1e-4
    assert bool((np.abs(no_bc - val) > bc.adam_tol(val, err))[moved].all())


def test_chain_case_list_covers_the_issue_shapes():
    cs = bc.CHAIN_CASES
    for key, want in (("H", {32, 96, 256}), ("in_dim", {17, 23, 65}), ("n", {1, 31, 33, 100, 512}), ("nets", {1, 3}), ("n_sel", {1, 2})):
        assert {c[key] for c in cs} == want, key
    assert {c["ld_pad"] == 0 for c in cs} == {True, False} and all(c["A"] <= 8 for c in cs)


@pytest.mark.parametrize("cid", bc.ids(bc.CHAIN_CASES))
def test_chain_layered_check_passes_a_float32_emulation_with_few_flagged_elements(cid):
    """the band arithmetic alone: a float32 emulation of the critic chain passes the layered check, under 2 % of each buffer lie
    where the band reaches a rounding boundary, and the accumulations measure at or below the recorded C_Q; one flipped mantissa
    bit, one wrong zero and one stale row are all caught"""
    case = bc._ALL[cid]
    inp = bc.chain_inputs(case)
    dev, worst = bc.emulate_critic_saves(case, inp)
    assert worst <= bc.MEASURED["C_Q"], f"{cid}: the accumulations measure {worst:.2f}, recorded {bc.MEASURED['C_Q']}"
    share = bc.check_critic_saves(case, inp, dev)
    assert all(v < 0.02 for v in share.values()), f"{cid}: flagged shares {share}"
    n, e = case["n"], case["nets"] - 1
    for key, row in (("H1T", 1), ("H2T", 5), ("DZ1T", 7), ("DZ2T", 2)):
        bad = {k: v.copy() for k, v in dev.items()}
        col = int(np.argmax(bad[key][e][row, :n] != 0)) if key != "DZ2T" else n - 1
        bad[key][e][row, col] = bad[key][e][row, col] ^ 1 if bad[key][e][row, col] else 0x3C00
        with pytest.raises(AssertionError):
            bc.check_critic_saves(case, inp, bad)
    bad = {k: v.copy() for k, v in dev.items()}
    bad["Q"][e][n - 1] *= np.float32(1.0 + 2.0 ** -14)
    bad["Q"][e][n - 1] += np.float32(1e-3)
    with pytest.raises(AssertionError):
        bc.check_critic_saves(case, inp, bad)


def _truncate(x):
    """float32 -> bf16 by dropping the low 16 bits (the WRONG rounding)"""
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def test_subtle_arithmetic_errors_lie_outside_the_bounds():
    """errors far below the sequence tests' 2 %: a re-rounding that truncates leaves the exact-kind bound in most weight elements,
    and a dz1 that truncates fails the layered check"""
    cid = next(c["id"] for c in bc.GRAD_CASES if (c["H"], c["n"]) == (64, 255))
    case, inp, ref = bc.load(cid, "exact")
    c = ref["loss"]["c"]
    for seg, dz, B in (("w1", inp["DZ1"], np.broadcast_to(inp["X"], (case["nets"],) + inp["X"].shape)), ("w2", inp["DZ2"], inp["H1"])):
        s_wrong = _truncate((c[..., None] * dz.astype(F64)).astype(F32)).astype(F64)
        wrong = np.einsum("ekm,ekn->emn", s_wrong, B.astype(F64))
        g, S, extra = ref[seg]
        assert float((np.abs(wrong - g) > bc.bound("exact", seg, S, extra)).mean()) > 0.5, seg
    cc = bc._ALL[bc.CLOSING_CASE]
    cin = bc.chain_inputs(cc)
    dev, _ = bc.emulate_critic_saves(cc, cin)
    i, H, n = cc["in_dim"], cc["H"], cc["n"]
    for e in range(cc["nets"]):   # dz1 again from the emulated stages, truncated
        _, _, W2, _, W3, _ = (a.astype(F32) for a in bc.net_parts(cin["critics"][e], i, H, 1))
        h1, h2 = bc.bf16_widen(dev["H1T"][e][:, :n].T), bc.bf16_widen(dev["H2T"][e][:, :n].T)
        dz2 = np.where(h2 > 0, W3[0][None, :], F32(0.0)).astype(F32)
        dz1 = np.where(h1 > 0, _truncate(bc._chain32(dz2, W2.T.copy())), F32(0.0)).astype(F32)
        dev["DZ1T"][e][:, :n] = bc.bf16_bits(dz1).T
    with pytest.raises(AssertionError, match="DZ1uT"):
        bc.check_critic_saves(cc, cin, dev)
