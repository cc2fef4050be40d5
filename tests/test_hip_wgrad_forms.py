"""GPU: every fp32 weight-gradient launch form (ssac_mlp_wgrad_fc12 / _all / _all_scaled / _all_lossfold / _all_actor,
ssac_mlp_layer_wgrad, ssac_head_wgrad, ssac_linear_wgrad_splitk + ssac_reduce_slices) through the C ABI, per element against the
float64 references of wgrad_cases.py: bit for bit on grid inputs in BOTH forced forms, under the CPU-derived bound on Gaussian
inputs with planted rows; the automatic form equals a forced one, the lean kernel equals the general one and the rebuilt dz2u the
stored one, bit for bit; Adam / Polyak against a float64 Adam built from the control block; sentinels behind every output.
Inputs, references and tolerances: wgrad_cases.py; the launch harness: wgrad_launch.py.  One case id names one entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_cases as wc
from wgrad_launch import DEV, SENT, Launch, _check_grads, _check_lossfold, _dev, _sent, _tail_ok, switches_restored

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture(autouse=True)
def _forms_restored(ssa):
    with switches_restored(ssa):
        yield


def _same(a, b, keys):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys if k in a)


@pytest.mark.parametrize("cid", wc.ids([c for c in wc.GRAD_CASES if c["entry"] in wc.MERGED]))
def test_merged_launch_gradient_store(ssa, cid):
    case = wc._ALL[cid]
    keys = ("grads", "sumsq", "partials", "td_out")
    nulls = (False, True) if case["dz2"] == "null" else (False,)
    for kind in wc.kinds(case):
        _, inp, ref = wc.load(cid, kind)
        L = Launch(ssa, case, inp)
        runs = {}
        for null in nulls:
            for variant in (1, 2):
                what = f"{cid} [{kind}, variant {variant}{', dz2u rebuilt' if null else ''}]"
                got = runs[(variant, null)] = L.run(variant=variant, dz2_null=null)
                _check_grads(L, got, ref, kind, what)
                if case["entry"] == "lossfold":
                    _check_lossfold(L, got, kind, what)
            if not wc.small_applies(case):   # an odd row count: the latency form declines, the 64 x 64 form runs
                assert _same(runs[(1, null)], runs[(2, null)], keys), f"{cid}: variant 2 must decline {case['n']} rows"
            if kind == "gauss":
                auto = L.run(variant=0, dz2_null=null)
                assert _same(auto, runs[(1, null)], keys) or _same(auto, runs[(2, null)], keys), \
                    f"{cid}: the automatic form equals neither forced form{' (dz2u rebuilt)' if null else ''}"
                general = L.run(variant=1, lean=0, dz2_null=null)
                assert _same(general, runs[(1, null)], keys), f"{cid}: lean and general kernel differ"
        if len(nulls) == 2 and kind == "gauss":
            for variant in (1, 2):
                assert _same(runs[(variant, False)], runs[(variant, True)], keys), f"{cid}: stored and rebuilt dz2u differ (variant {variant})"


@pytest.mark.parametrize("cid", wc.ids([c for c in wc.GRAD_CASES if c["entry"] not in wc.MERGED]))
def test_single_layer_launch_gradient_store(ssa, cid):
    case = wc._ALL[cid]
    for kind in ("grid", "gauss"):
        _, inp, ref = wc.load(cid, kind)
        L = Launch(ssa, case, inp)
        got = L.run()
        _check_grads(L, got, ref, kind, f"{cid} [{kind}]")
        if kind == "gauss" and case["entry"] != "head":
            assert _same(L.run(lean=0), got, ("grads", "sumsq")), f"{cid}: lean and general kernel differ"


def test_lossfold_refuses_more_than_4096_rows(ssa):
    lib = ssa._lib.lib
    desc = ssa._lib.MlpDesc(0, 64, 1, 4, 4, 1)
    one = torch.zeros(8, device=DEV).data_ptr()   # (refused on the host: nothing is launched, nothing read)
    args = [C.byref(desc), one, 4, 0, one, one, one, one, 0, one, one, 0, 0, 0, 0, 1.0, one]
    rest = [one, one, 0, one, 0, 0, 0, 0, 0, 0.0, 0, ssa.engine.stream()]
    assert lib.ssac_mlp_wgrad_all_lossfold(*args, 4097, *rest) != 0
    assert "4096" in lib.ssac_last_error().decode()


@pytest.mark.parametrize("cid", wc.ids(wc.SPLITK_CASES))
def test_linear_wgrad_splitk_and_reduce(ssa, cid):
    lib, st = ssa._lib.lib, ssa.engine.stream()
    for kind in ("grid", "gauss"):
        case, inp, ref = wc.load(cid, kind)
        M, N, n = case["M"], case["N"], case["n"]
        slices = ref["pw"].shape[0]
        assert slices == -(-n // case["rps"])
        dY, X = _dev(inp["dY"])[1], _dev(inp["X"])[1]
        pw, pb, ow, ob = _sent(slices * M * N), _sent(slices * M), _sent(M * N), _sent(M)
        ssa._lib.check(lib.ssac_linear_wgrad_splitk(dY.data_ptr(), case["ldy"], X.data_ptr(), case["ldx"], pw.data_ptr(), pb.data_ptr(),
                                                    M, N, n, case["rps"], st))
        ssa._lib.check(lib.ssac_reduce_slices(pw.data_ptr(), slices, M * N, ow.data_ptr(), st))
        ssa._lib.check(lib.ssac_reduce_slices(pb.data_ptr(), slices, M, ob.data_ptr(), st))
        for buf, numel, what in ((pw, slices * M * N, "partial_w"), (pb, slices * M, "partial_b"), (ow, M * N, "dW"), (ob, M, "db")):
            _tail_ok(buf, numel, f"{cid}: {what}")
        for have, g, S, seg, what in (
                (pw[:slices * M * N], ref["pw"], ref["sw"], "w", "partial_w"), (pb[:slices * M], ref["pb"], ref["sb"], "b", "partial_b"),
                (ow[:M * N], ref["pw"].sum(0), ref["sw"].sum(0), "w", "reduced dW"), (ob[:M], ref["pb"].sum(0), ref["sb"].sum(0), "b", "reduced db")):
            have = have.cpu().numpy().astype(np.float64).reshape(g.shape)
            if kind == "grid":
                assert np.array_equal(have, g), f"{cid}: {what} differs from the exact sums"
            else:
                assert bool((np.abs(have - g) <= wc.bound(seg, S)).all()), f"{cid}: {what} beyond its bound"


@pytest.mark.parametrize("cid", wc.ids(wc.ADAM_CASES))
def test_adam_and_polyak_epilogues(ssa, cid):
    case = wc._ALL[cid]
    base = {k: case[k] for k in wc._c("x", 2)}
    inp = wc.make_inputs(dict(base, id=cid), "grid")
    ref = wc.reference(base, inp)
    L = Launch(ssa, case, inp, adam=case)
    null = case["dz2"] == "null"
    ctl = wc.adam_ctl(case)
    nets, stride = case["nets"], L.stride
    old = dict(zip(("m", "v", "target"), wc.adam_state(case, (nets, stride))), p=inp["params"])
    merged = case["entry"] in wc.MERGED
    runs = {}
    for variant in ((1, 2) if merged else (0,)):
        got = runs[variant] = L.run(variant=variant, dz2_null=null)
        what = f"{cid} [variant {variant}]"
        got["p"] = got["params"]
        seeded = old
        for k in ("m", "v", "p") + (("target",) if case["target"] else ()):
            before = old[k].copy()
            before[:, L.off[5] + case["out"]:] = SENT
            L.untouched_ok(got[k], f"{what}: {k}", before=before)
        sums = L.sumsq_rows(got["sumsq"])
        for slot in range(L.ns):
            g2 = {l: 0.0 for l in L.layers()}
            for s in L.segs():
                g = ref[s][0][slot]
                sl = wc.seg_slices(case)[s]
                o = {k: seeded[k][L.ids[slot], sl].reshape(g.shape) for k in ("m", "v", "p", "target")}
                r = wc.adam_ref(ctl, o["p"], g, o["m"], o["v"], o["target"] if case["target"] else None)
                for k in ("m", "v", "p") + (("target",) if case["target"] else ()):
                    have = L.seg_of(got[k], slot, s).astype(np.float64).reshape(g.shape)
                    bad = np.abs(have - r[k]) > wc.adam_tol(o[k], r[k])
                    assert not bad.any(), f"{what}: {k} of {s}, slot {slot} (net {L.ids[slot]}): {int(bad.sum())} of {bad.size} off"
                g2[int(s[1]) - 1] += float((g * g).sum())
            have2, want2 = sum(sums[l][slot] for l in L.layers()), sum(g2.values())
            assert abs(have2 - want2) <= 1e-5 * want2, f"{what}: sumsq of slot {slot}: {have2!r} vs {want2!r}"
        if case["entry"] == "lossfold":
            _check_lossfold(L, got, "grid", what)
        if case["entry"] == "actor":
            assert int(got["done"][0]) == 0 and bool((got["done"][1:] == 0).all()), f"{what}: the done counter is not back at zero"
            loss = 0.75 - wc.ACTOR_INV * float(L.a_parts.astype(np.float64).sum()) / case["n"]
            gn = float(np.sqrt(sum(float(v_[0]) for v_ in sums.values())))
            assert abs(float(got["logs"][0]) - loss) <= wc.log_tol(L.a_parts) and abs(float(got["logs"][1]) - gn) <= 1e-5 * gn, f"{what}: folded logs"
            _tail_ok(got["logs"], 2, "logs")
    if merged:
        keys = ("m", "v", "params", "target", "sumsq", "partials", "td_out")
        auto = L.run(variant=0, dz2_null=null)
        assert _same(auto, runs[1], keys) or _same(auto, runs[2], keys), f"{cid}: the automatic form equals neither forced form"
        assert _same(L.run(variant=1, lean=0, dz2_null=null), runs[1], keys), f"{cid}: lean and general kernel differ"
