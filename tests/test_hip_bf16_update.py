"""GPU: the bf16 critic update's kernels (csrc/ssac_bf16.hip) through the C ABI, per element against the float64 references of
bf16_cases.py: ssac_bf16_wgrad_lossfold in gradient mode (bit for bit on grid inputs, under the CPU-derived bounds on Gaussian
inputs with planted rows, pad-column contract, guards, refusals) and in Adam mode with and without Polyak (float64 Adam built from
the control block, shadows exact from the device's own masters), ssac_bf16_polyak, the critic saves of ssac_bf16_chain_update layer
by layer from the device's own previous stage in both launch forms, and chain + weight gradient end to end.
Inputs, references and tolerances: bf16_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_cases as bc
from wgrad_cases import SEGS, adam_ctl, layout, log_tol, seg_shapes, seg_slices, sumsq_tol, td_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT, TAIL, GAP = bc.SENT, bc.TAIL, bc.GAP
F64 = np.float64


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _dev(a):
    """device copy of a float32 host array followed by TAIL sentinel words"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.full((a.size + TAIL,), SENT, device=DEV)
    buf[:a.size] = torch.from_numpy(a).to(DEV)
    return buf


def _dev16(bits):
    """device copy of uint16 words followed by TAIL words of SHADOW_SENT"""
    a = np.concatenate([np.ascontiguousarray(bits, np.uint16).reshape(-1), np.full(TAIL, bc.SHADOW_SENT, np.uint16)])
    return torch.from_numpy(a.view(np.int16).copy()).to(DEV)


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _sent(numel):
    return torch.full((numel + TAIL,), SENT, device=DEV)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seg(case, arena, e, seg):
    _, stride = layout(case["in_dim"], case["H"], 1)
    return arena[:case["nets"] * stride].reshape(case["nets"], stride)[e, seg_slices(case)[seg]].reshape(seg_shapes(case)[seg])


def _desc(ssa, ptr, case, out=1):
    _, stride = layout(case["in_dim"], case["H"], out)
    return ssa._lib.MlpDesc(ptr, stride, case["nets"], case["in_dim"], case["H"], out)


def saves_of(case, inp, pad_bits=0):
    """the five fragment-major transposed buffers of (case, inputs): uint16 words"""
    n, h, i, nets = case["n"], case["H"], case["in_dim"], case["nets"]
    bp = bc.bp_of(n)
    out = dict(XT=bc.to_frag(inp["X"].T, bc.xt_rows(i), bp, pad_bits))
    for k, src in (("H1T", "H1"), ("H2T", "H2"), ("DZ2T", "DZ2"), ("DZ1T", "DZ1")):
        out[k] = np.concatenate([bc.to_frag(inp[src][e].T, h, bp, pad_bits) for e in range(nets)])
    return out


def shadow_before(case, nets=None):
    """a shadow whose every word the Adam epilogue / Polyak must write holds SHADOW_SENT; W1's K-pad columns are zero"""
    stride, o1, o2, o2t, o3, k1p = bc.shadow_geom(case["in_dim"], case["H"])
    one = np.full(stride, bc.SHADOW_SENT, np.uint16)
    w1 = np.full((case["H"], k1p), bc.SHADOW_SENT, np.uint16)
    w1[:, case["in_dim"]:] = 0
    one[o1:o2] = 0
    idx = bc.frag_index(case["H"], k1p).reshape(-1)
    one[o1:o2][idx] = w1.reshape(-1)
    return np.tile(one, case["nets"] if nets is None else nets)


class Wgrad:
    """the device buffers of one (case, inputs) and the ssac_bf16_wgrad_lossfold launch"""

    def __init__(self, ssa, case, inp, kind, saves=None):
        self.ssa, self.case, self.inp, self.kind = ssa, case, inp, kind
        c = case
        self.off, self.stride = layout(c["in_dim"], c["H"], 1)
        self.sh_stride = bc.shadow_geom(c["in_dim"], c["H"])[0]
        offs = (C.c_int64 * 4)()
        assert ssa._lib.lib.ssac_bf16_layout(c["in_dim"], c["H"], 1, offs) == self.sh_stride
        assert list(offs) == list(bc.shadow_geom(c["in_dim"], c["H"])[1:5])
        self.tiles = bc.wgrad_tiles(c)
        assert ssa._lib.lib.ssac_bf16_wgrad_tiles(C.byref(_desc(ssa, 0, c))) == self.tiles
        self.ss_stride = self.tiles + GAP
        self.saves = saves
        lf = inp["lf"]
        self.keep = {k: _dev(lf[k]) for k in ("Q", "td", "q_t", "logp", "rew", "done", "weight") if k in lf}
        self.keep["la"] = _dev(np.array([lf["log_alpha"]]))
        pa = bc.popart_struct(c, kind)
        self.pop = ssa.engine.DeviceStruct(ssa._lib.PopArtState(0.3, 2.0, pa[0], pa[1], 5, 2, 1, 0, 1e-2), torch.device(DEV)) if pa else None
        self.pop_flag = pa[2] if pa else 0

    def run(self, pad_bits=0, adam=None, late=None):
        """gradient mode (adam None) or Adam mode; late: None = tau in the launch, else the bits of the late-bound word"""
        ssa, c, inp, k = self.ssa, self.case, self.inp, self.keep
        lib, st = ssa._lib.lib, ssa.engine.stream()
        n, nets = c["n"], c["nets"]
        total = nets * self.stride
        sv = self.saves if self.saves is not None else saves_of(c, inp, pad_bits)
        dsv = {kk: _dev16(v) for kk, v in sv.items()}
        params = _dev(inp["params"])
        out = dict(params=params)
        live = np.zeros((nets, self.stride), bool)
        live[:, :self.off[5] + 1] = True
        if adam is None:
            shadow0 = np.concatenate([bc.shadow_of(inp["params"][e], c["in_dim"], c["H"], fill=bc.SHADOW_SENT) for e in range(nets)])
            grads = out["grads"] = _sent(total)
            m, v = out["m"], out["v"] = _sent(total), _sent(total)
            f = adam_ctl(dict(seeded=0, wd=0.0))
            tgt = tsh = None
        else:
            shadow0 = shadow_before(c)
            grads = None
            st_ = bc.adam_state(adam, (nets, self.stride))
            arrs = [np.where(live, a, np.float32(SENT)) for a in st_]
            m, v = out["m"], out["v"] = _dev(arrs[0]), _dev(arrs[1])
            tgt = tsh = None
            if adam["target"]:
                tgt, tsh = out["target"], out["tshadow"] = _dev(arrs[2]), _dev16(shadow_before(c))
            f = adam_ctl(adam)
        self.shadow0 = shadow0
        shadow = out["shadow"] = _dev16(shadow0)
        cs = ssa._lib.AdamCtl(f["lr"], f["beta1"], f["beta2"], f["eps"], f["wd"], f["step_size"], f["bc2_sqrt"], 1.0, f["step"],
                              (C.c_int32 * 3)(0, 0, 0), bc.LR, bc.BETA1, bc.BETA2)
        ctl = self.ctl = ssa.engine.DeviceStruct(cs, torch.device(DEV))
        ss = out["sumsq"] = _sent(GAP + nets * self.ss_stride)
        parts, td_out = out["partials"], out["td_out"] = _sent(2 * nets), _sent(n)
        spec = None
        if "q_t" in inp["lf"]:
            spec = self.spec = ssa._lib.TdSpec(_p(k["q_t"]), _p(k["logp"]), _p(k["rew"]), _p(k["done"]), _p(k["la"]), td_out.data_ptr(),
                                               float(inp["lf"]["gamma"]), 2, 1, 0)
        fold = None
        if late is not None:
            word = self.word = torch.tensor([late], dtype=torch.int64, device=DEV).to(torch.int32)
            fold = self.fold = ssa._lib.LogFold(0, 0, 0, 0, 0, word.data_ptr())
        desc = _desc(ssa, params.data_ptr(), c)
        rc = lib.ssac_bf16_wgrad_lossfold(
            C.byref(desc), shadow.data_ptr(), _p(dsv["XT"]), _p(dsv["H1T"]), _p(dsv["H2T"]), _p(dsv["DZ2T"]), _p(dsv["DZ1T"]),
            _p(k["Q"]), _p(k.get("td")), C.addressof(spec) if spec else 0, _p(k.get("weight")), self.pop.ptr if self.pop else 0,
            self.pop_flag, float(c["denom"]), parts.data_ptr(), n, m.data_ptr(),
            v.data_ptr(), ctl.ptr, _p(grads), ss.data_ptr() + 4 * GAP, self.ss_stride, _p(tgt), _p(tsh),
            bc.TAU if (tgt is not None and late is None) else 0.0, C.addressof(fold) if fold else 0, st)
        ssa._lib.check(rc)
        torch.cuda.synchronize()
        res = {kk: (_host16(vv) if vv.dtype == torch.int16 else vv.cpu().numpy()) for kk, vv in out.items()}
        for kk, vv in dsv.items():   # the launch reads its saves only
            assert np.array_equal(_host16(vv)[:-TAIL], sv[kk]), f"{kk} changed"
        return res

    def seg_of(self, arena, e, seg):
        return _seg(self.case, arena, e, seg)

    def arena_guard(self, arena, what, before=None, written=True):
        """every word outside the six segments (all words if not `written`): the value before (default: the sentinel)"""
        nets = self.case["nets"]
        live = np.zeros((nets, self.stride), bool)
        if written:
            live[:, :self.off[5] + 1] = True
        a = arena[:nets * self.stride].reshape(nets, self.stride)
        want = np.full_like(a, SENT) if before is None else np.asarray(before, np.float32).reshape(nets, self.stride)
        assert np.array_equal(_bits(a[~live]), _bits(want[~live])), f"{what}: words outside the launch's segments changed"
        assert np.array_equal(arena[nets * self.stride:], np.full(TAIL, SENT, np.float32)), f"{what}: written past its end"

    def sumsq_rows(self, ss):
        nets = self.case["nets"]
        rows = ss[GAP:GAP + nets * self.ss_stride].reshape(nets, self.ss_stride)
        assert bool((ss[:GAP] == SENT).all()) and bool((rows[:, self.tiles:] == SENT).all()) and bool((ss[GAP + nets * self.ss_stride:] == SENT).all()), \
            "sumsq: written outside its slots"
        assert bool(np.isfinite(rows[:, :self.tiles]).all()) and bool((rows[:, :self.tiles] != SENT).all()), "sumsq: a slot was not written"
        return rows[:, :self.tiles].astype(F64).sum(1)


def _check_lossfold(L, got, ref, kind, what):
    c, inp, s = L.case, L.inp, ref["loss"]
    n, nets = c["n"], c["nets"]
    assert np.array_equal(got["partials"][2 * nets:], np.full(TAIL, SENT, np.float32)), f"{what}: partials written past the end"
    assert np.array_equal(got["td_out"][n:], np.full(TAIL, SENT, np.float32)), f"{what}: td_out written past the end"
    parts = got["partials"][:2 * nets].reshape(nets, 2).astype(F64)
    for e in range(nets):
        for j, terms in ((0, s["werr2"][e]), (1, s["err"][e])):
            if kind == "grid":
                assert parts[e, j] == terms.sum(), f"{what}: partials[{e}][{j}] on the grid"
            assert abs(parts[e, j] - terms.sum()) / n <= log_tol(terms), f"{what}: partials[{e}][{j}] {parts[e, j]!r} vs {terms.sum()!r}"
    if "q_t" in inp["lf"]:
        td = got["td_out"][:n].astype(F64)
        assert bool((np.abs(td - s["td"]) <= (0.0 if kind == "grid" else td_tol(inp["lf"]))).all()), f"{what}: td_out"
    else:
        assert bool((got["td_out"] == SENT).all()), f"{what}: td_out written though td was given"


def _check_grads(L, got, ref, kind, what):
    c = L.case
    L.arena_guard(got["grads"], f"{what}: grads")
    for k in ("m", "v"):
        L.arena_guard(got[k], f"{what}: {k}", written=False)
    assert np.array_equal(_bits(got["params"][:-TAIL]), _bits(L.inp["params"].reshape(-1))), f"{what}: gradient mode changed the parameters"
    assert np.array_equal(got["shadow"][:-TAIL], L.shadow0) and bool((got["shadow"][-TAIL:] == bc.SHADOW_SENT).all()), f"{what}: gradient mode changed the shadow"
    sums = L.sumsq_rows(got["sumsq"])
    for e in range(c["nets"]):
        g2 = tol = 0.0
        for s in SEGS:
            g, S, extra = (a[e] for a in ref[s])
            have = L.seg_of(got["grads"], e, s).astype(F64).reshape(g.shape)
            if kind == "grid":
                d = np.zeros_like(g)
                assert np.array_equal(have, g), f"{what}: {s} of net {e} differs from the exact sums in {int((have != g).sum())} of {g.size} elements"
            else:
                d = bc.bound(kind, s, S, extra)
                ratio = np.abs(have - g) / np.maximum(d, 1e-300)
                assert float(ratio.max()) <= 1.0, f"{what}: {s} of net {e} off by {float(ratio.max()):.3g} bounds at {np.unravel_index(ratio.argmax(), ratio.shape)}"
            g2 += float((g * g).sum())
            tol += sumsq_tol(g, d)
        assert abs(sums[e] - g2) <= tol, f"{what}: sumsq of net {e}: {sums[e]!r} vs {g2!r}"
    _check_lossfold(L, got, ref, kind, what)


@pytest.mark.parametrize("cid", bc.ids(bc.GRAD_CASES))
def test_wgrad_gradient_mode_per_element(ssa, cid):
    case = bc._ALL[cid]
    for kind in bc.kinds(case):
        _, inp, ref = bc.load(cid, kind)
        L = Wgrad(ssa, case, inp, kind)
        _check_grads(L, L.run(), ref, kind, f"{cid} [{kind}]")


@pytest.mark.parametrize("kind", ["grid", "exact", "general"])
def test_wgrad_results_do_not_depend_on_finite_pad_columns(ssa, kind):
    """bf_buffers reuses the saves across calls with the same Bp and nothing ever writes the columns [n_rows, Bp): finite stale
    values there must not reach any output"""
    cid = bc.PAD_CASES[kind]
    case, inp, ref = bc.load(cid, kind)
    L = Wgrad(ssa, case, inp, kind)
    clean, stale = L.run(pad_bits=0), L.run(pad_bits=bc.PAD_ONE)
    _check_grads(L, stale, ref, kind, f"{cid} [{kind}, stale pads]")
    for k in ("grads", "sumsq", "partials", "td_out"):
        assert np.array_equal(_bits(clean[k]), _bits(stale[k])), f"{cid} [{kind}]: {k} depends on the pad columns"


def test_wgrad_refusals(ssa):
    lib = ssa._lib.lib
    # refused on the host, nothing is launched; should a refusal ever regress, every pointer still names live zeroed memory
    # large enough for what the call describes (hidden 32, up to 8208 batch columns)
    keep = torch.zeros(32 * 8208 + 4096, device=DEV)
    one = keep.data_ptr()

    def call(desc, n_rows=16, grads=0, target=0, tshadow=0):
        return lib.ssac_bf16_wgrad_lossfold(C.byref(desc), one, one, one, one, one, one, one, one, 0, 0, 0, 0, 1.0, one, n_rows, one, one,
                                            one, grads, one, 3, target, tshadow, 0.25, 0, ssa.engine.stream())
    good = ssa._lib.MlpDesc(one, layout(16, 32, 1)[1], 1, 16, 32, 1)
    assert call(good, n_rows=8193) != 0 and "8192" in lib.ssac_last_error().decode()
    assert call(ssa._lib.MlpDesc(one, layout(16, 32, 2)[1], 1, 16, 32, 2)) != 0 and "single-output" in lib.ssac_last_error().decode()
    assert call(good, target=one) != 0 and "shadow" in lib.ssac_last_error().decode()
    assert call(good, grads=one, target=one, tshadow=one) != 0 and "gradient mode" in lib.ssac_last_error().decode()
    torch.cuda.synchronize()


def _shadow_parts(case, words):
    """(W1 incl. K pad, W2, W2^T, W3, tail) of one net's shadow words, row-major bit patterns"""
    stride, o1, o2, o2t, o3, k1p = bc.shadow_geom(case["in_dim"], case["H"])
    h = case["H"]
    return (bc.from_frag(words[o1:o2], h, k1p), bc.from_frag(words[o2:o2t], h, h), bc.from_frag(words[o2t:o3], h, h), words[o3:o3 + h],
            words[o3 + h:stride])


def _check_shadow(c, words, arena, what):
    """every shadow word equals bf16 of the DEVICE's master in `arena`, W1's K pad is zero, nothing else changed"""
    sh_stride = bc.shadow_geom(c["in_dim"], c["H"])[0]
    assert bool((words[c["nets"] * sh_stride:] == bc.SHADOW_SENT).all()), f"{what}: written past its end"
    for e in range(c["nets"]):
        w1, w2, w2t, w3, tail = _shadow_parts(c, words[e * sh_stride:(e + 1) * sh_stride])
        P1, P2, P3 = (bc.bf16_bits(_seg(c, arena, e, s)) for s in ("w1", "w2", "w3"))
        assert np.array_equal(w1[:, :c["in_dim"]], P1), f"{what}: W1 of net {e} is not bf16 of the master ({int((w1[:, :c['in_dim']] != P1).sum())} words)"
        assert not w1[:, c["in_dim"]:].any(), f"{what}: W1's K pad of net {e} is not zero"
        assert np.array_equal(w2, P2), f"{what}: W2 of net {e}: {int((w2 != P2).sum())} words differ from bf16 of the master"
        assert np.array_equal(w2t, P2.T), f"{what}: W2^T of net {e}: {int((w2t != P2.T).sum())} words differ from bf16 of the master"
        assert np.array_equal(w3, P3.reshape(-1)), f"{what}: W3 of net {e}"
        assert bool((tail == bc.SHADOW_SENT).all()), f"{what}: the stride's padding of net {e} changed"


@pytest.mark.parametrize("cid", bc.ids(bc.ADAM_CASES))
def test_wgrad_adam_mode_and_polyak(ssa, cid):
    case = bc._ALL[cid]
    inp = bc.make_inputs(case, "grid")
    ref = bc.reference(case, inp)
    L = Wgrad(ssa, case, inp, "grid")
    ctl = adam_ctl(case)
    nets = case["nets"]
    old = dict(zip(("m", "v", "target"), bc.adam_state(case, (nets, L.stride))), p=inp["params"])
    keys = ("m", "v", "p") + (("target",) if case["target"] else ())
    got = L.run(adam=case)
    got["p"] = got["params"]
    what = cid
    for k in keys:
        before = old[k].copy()
        before[:, L.off[5] + 1:] = SENT
        L.arena_guard(got[k], f"{what}: {k}", before=before)
    sums = L.sumsq_rows(got["sumsq"])
    for e in range(nets):
        g2 = tol = 0.0
        for s in SEGS:
            g = ref[s][0][e]
            sl = seg_slices(case)[s]
            o = {k: old[k][e, sl].reshape(g.shape) for k in ("m", "v", "p", "target")}
            r = bc.adam_ref(ctl, o["p"], g, o["m"], o["v"], o["target"] if case["target"] else None)
            for k in keys:
                have = L.seg_of(got[k], e, s).astype(F64).reshape(g.shape)
                bad = np.abs(have - r[k][0]) > bc.adam_tol(*r[k])
                assert not bad.any(), f"{what}: {k} of {s}, net {e}: {int(bad.sum())} of {bad.size} off, worst " \
                                      f"{float((np.abs(have - r[k][0]) / bc.adam_tol(*r[k])).max()):.3g} tolerances"
            g2 += float((g * g).sum())
            tol += sumsq_tol(g, np.zeros_like(g))   # (the gradient is exact on the grid)
        assert abs(sums[e] - g2) <= tol, f"{what}: sumsq of net {e}: {sums[e]!r} vs {g2!r}"
    _check_lossfold(L, got, ref, "grid", what)
    _check_shadow(case, got["shadow"], got["p"], f"{what}: shadow")
    if not case["target"]:
        return
    _check_shadow(case, got["tshadow"], got["target"], f"{what}: target shadow")
    # the late-bound form: the same tau as bits of a device word gives the same update, zero bits leave the target alone
    same = ("m", "v", "params", "shadow", "sumsq", "partials", "td_out")
    tau_bits = int(np.float32(bc.TAU).view(np.uint32))
    late = L.run(adam=case, late=tau_bits)
    for k in same + ("target", "tshadow"):
        assert np.array_equal(late[k].view(np.uint8), got[k].view(np.uint8)), f"{what}: late-bound tau: {k} differs from the direct form"
    off = L.run(adam=case, late=0)
    for k in same:
        assert np.array_equal(off[k].view(np.uint8), got[k].view(np.uint8)), f"{what}: late word 0: {k} differs from the direct form"
    before = np.where(np.arange(L.stride)[None, :] < L.off[5] + 1, old["target"], np.float32(SENT))
    L.arena_guard(off["target"], f"{what}: late word 0: target", before=before, written=False)
    assert np.array_equal(off["tshadow"][:-TAIL], shadow_before(case)), f"{what}: late word 0: the target's shadow changed"


@pytest.mark.parametrize("cid", bc.ids(bc.POLYAK_CASES))
def test_polyak_masters_and_target_shadow(ssa, cid):
    case = bc._ALL[cid]
    g = bc._rng(case, "polyak")
    nets = case["nets"]
    off, stride = layout(case["in_dim"], case["H"], 1)
    T0 = np.full((nets, stride), SENT, np.float32)
    S0 = np.full((nets, stride), SENT, np.float32)
    T0[:, :off[5] + 1] = g.standard_normal((nets, off[5] + 1))
    S0[:, :off[5] + 1] = g.standard_normal((nets, off[5] + 1))
    S0[:, off[5] + 1:] = 3.0   # (a padding of its own: a kernel that copied the source's padding would show)
    T, S, tsh = _dev(T0), _dev(S0), _dev16(shadow_before(case))
    tau = 0.005
    ssa._lib.check(ssa._lib.lib.ssac_bf16_polyak(C.byref(_desc(ssa, T.data_ptr(), case)), C.byref(_desc(ssa, S.data_ptr(), case)), tau,
                                                 tsh.data_ptr(), ssa.engine.stream()))
    torch.cuda.synchronize()
    Th, Sh = T.cpu().numpy(), S.cpu().numpy()
    assert np.array_equal(_bits(Sh), _bits(np.concatenate([S0.reshape(-1), np.full(TAIL, SENT, np.float32)]))), f"{cid}: the source changed"
    assert bool((Th[nets * stride:] == SENT).all()), f"{cid}: the target was written past its end"
    t0, s0 = T0.astype(F64), S0.astype(F64)
    tau32 = np.float32(tau)   # the kernel's two factors: tau and 1 - tau as float32 numbers (one IEEE subtraction)
    want = t0 * float(np.float32(1.0) - tau32) + s0 * float(tau32)
    have = Th[:nets * stride].reshape(nets, stride).astype(F64)
    bad = np.abs(have - want) > bc.polyak_tol(t0, s0)
    assert not bad.any(), f"{cid}: {int(bad.sum())} target words (biases included) beyond 2^-23 (|T| + |S|)"
    # the stride's padding: the kernel blends EVERY word of a net's stride (ssac_mlp_layout's return value), so the padding is
    # written too -- with exactly the float32 blend of the two arenas' padding words, bit for bit (zero stays zero in a real arena)
    one32 = np.float32(1.0)
    pad_want = T0[:, off[5] + 1:] * (one32 - tau32) + S0[:, off[5] + 1:] * tau32
    assert np.array_equal(_bits(Th[:nets * stride].reshape(nets, stride)[:, off[5] + 1:]), _bits(pad_want)), f"{cid}: the stride's padding"
    assert bool((np.abs(have - t0)[:, :off[5] + 1] > 0).mean() > 0.9), f"{cid}: the target did not move"
    _check_shadow(case, _host16(tsh), Th, f"{cid}: target shadow")


# ------------------------------------------------------------------------------------------------ the chained launch
SAVE_SENT = bc.SHADOW_SENT   # (a finite bf16 value, 161.0: what the saves hold wherever the launch must not write)


def _shadow_sync(ssa, params, nets, in_dim, hidden, out_dim):
    """(device masters, device shadow) of an arena given as a (nets x stride) host array"""
    P = _dev(params)
    stride = int(ssa._lib.lib.ssac_bf16_layout(in_dim, hidden, out_dim, None))
    sh = torch.zeros(nets * stride, dtype=torch.int16, device=DEV)
    desc = ssa._lib.MlpDesc(P.data_ptr(), layout(in_dim, hidden, out_dim)[1], nets, in_dim, hidden, out_dim)
    ssa._lib.check(ssa._lib.lib.ssac_bf16_sync(C.byref(desc), sh.data_ptr(), ssa.engine.stream()))
    return P, sh, desc


def run_chain(ssa, case, inp, pc):
    """one ssac_bf16_chain_update launch (pc: the producer / consumer form with a zeroed hand-off); the saves come back both raw
    (fragment-major device words) and row-major"""
    lib = ssa._lib.lib
    S, A, H, n, nets, n_sel = case["S"], case["A"], case["H"], case["n"], case["nets"], case["n_sel"]
    i, bp, xr = S + A, bc.bp_of(case["n"]), bc.xt_rows(S + A)
    keep = [_shadow_sync(ssa, inp["actor"], 1, S, H, 2 * A), _shadow_sync(ssa, inp["targets"], case["n_targets"], i, H, 1),
            _shadow_sync(ssa, inp["critics"], nets, i, H, 1)]
    (Pa, sa, da), (Pt, st_, dt), (Pc, sc, dc) = keep
    Xa, eps, Xc = _dev(inp["Xa"]), _dev(inp["eps"]), _dev(inp["Xc"])
    x1 = np.full((n, i), SENT, np.float32)
    x1[:, :S] = inp["Xa"]
    x1sa, logp, Qt, Q = _dev(x1), _sent(n), _sent(n_sel * n), _sent(nets * n)
    ids = torch.tensor(inp["ids"], dtype=torch.int32, device=DEV)
    sv = {k: _dev16(np.full(nets * H * bp, SAVE_SENT, np.uint16)) for k in ("H1T", "H2T", "DZ2T", "DZ1T")}
    sv["XT"] = _dev16(np.full(xr * bp, SAVE_SENT, np.uint16))
    ho = torch.zeros(n * A, dtype=torch.int64, device=DEV) if pc else None
    ssa._lib.check(lib.ssac_bf16_chain_update(
        C.byref(da), sa.data_ptr(), Xa.data_ptr(), S, n, eps.data_ptr(), bc.LOG_STD_LO, bc.LOG_STD_HI, x1sa.data_ptr(), i, S,
        logp.data_ptr(), 0, C.byref(dt), st_.data_ptr(), ids.data_ptr(), n_sel, Qt.data_ptr(), C.byref(dc), sc.data_ptr(), Xc.data_ptr(),
        inp["ldxc"], Q.data_ptr(), sv["H1T"].data_ptr(), sv["H2T"].data_ptr(), sv["DZ2T"].data_ptr(), sv["DZ1T"].data_ptr(),
        sv["XT"].data_ptr(), 0, 0, _p(ho), ssa.engine.stream()))
    torch.cuda.synchronize()
    raw = {k: _host16(v) for k, v in sv.items()}
    for k, v in raw.items():
        assert bool((v[-TAIL:] == bc.SHADOW_SENT).all()), f"{k}: written past its end"
    out = dict(raw={k: v[:-TAIL].copy() for k, v in raw.items()}, x1sa=x1sa.cpu().numpy(), logp=logp.cpu().numpy(), Qt=Qt.cpu().numpy(),
               Qraw=Q.cpu().numpy())
    out["XT"] = bc.from_frag(out["raw"]["XT"], xr, bp)
    for k in ("H1T", "H2T", "DZ2T", "DZ1T"):
        out[k] = np.stack([bc.from_frag(out["raw"][k][e * H * bp:(e + 1) * H * bp], H, bp) for e in range(nets)])
    out["Q"] = out["Qraw"][:nets * n].reshape(nets, n)
    for P, host in ((Pa, inp["actor"]), (Pt, inp["targets"]), (Pc, inp["critics"])):
        assert np.array_equal(_bits(P.cpu().numpy()[:-TAIL]), _bits(host.reshape(-1))), "the chained launch changed a master arena"
    return out


def _check_chain(case, inp, got, what):
    S, A, n, i, nets, n_sel = case["S"], case["A"], case["n"], case["in_dim"], case["nets"], case["n_sel"]
    k1p = (i + 15) // 16 * 16
    try:
        share = bc.check_critic_saves(case, inp, got)
    except AssertionError as err:
        raise AssertionError(f"{what}: {err}") from None
    assert all(v < 0.02 for v in share.values()), f"{what}: flagged shares {share}"
    # pad columns of every save and the feature rows of XT beyond the tile's K1P keep what they held
    assert bool((got["XT"][:, n:] == SAVE_SENT).all()) and bool((got["XT"][k1p:] == SAVE_SENT).all()), f"{what}: XT written outside [0, K1P) x [0, n_rows)"
    for k in ("H1T", "H2T", "DZ2T", "DZ1T"):
        assert bool((got[k][:, :, n:] == SAVE_SENT).all()), f"{what}: {k} written in its pad columns"
    for k, numel in (("Qraw", nets * n), ("Qt", n_sel * n), ("logp", n), ("x1sa", n * i)):
        assert bool((got[k][numel:] == SENT).all()), f"{what}: {k} written past its end"
    # the target chain, at the forward test's stated tolerance only: a', log pi, and Qt from the DEVICE's [s'|a']
    x1 = got["x1sa"][:n * i].reshape(n, i)
    assert np.array_equal(_bits(x1[:, :S]), _bits(inp["Xa"])), f"{what}: the state columns of x1sa changed"
    sr = bc.sample_reference(case, inp)
    assert bool((np.abs(x1[:, S:].astype(F64) - sr["a"]) <= sr["a_tol"]).all()), f"{what}: a'"
    assert bool((np.abs(got["logp"][:n].astype(F64) - sr["logp"]) <= sr["logp_tol"]).all()), f"{what}: log pi"
    for slot, net in enumerate(inp["ids"]):
        ref = bc.forward_emulation(inp["targets"][net], i, case["H"], 1, x1)[:, 0]
        dv = np.abs(got["Qt"][slot * n:(slot + 1) * n].astype(F64) - ref).max()
        assert dv <= bc.FWD_RTOL * np.abs(ref).max() + bc.FWD_ATOL, f"{what}: Qt of slot {slot} (net {net}) off by {dv:.3g}"


@pytest.mark.parametrize("cid", bc.ids(bc.CHAIN_CASES))
def test_chain_critic_saves_layer_by_layer_in_both_forms(ssa, cid):
    case = bc._ALL[cid]
    inp = bc.chain_inputs(case)
    plain = run_chain(ssa, case, inp, pc=False)
    _check_chain(case, inp, plain, f"{cid} [plain]")
    pc = run_chain(ssa, case, inp, pc=True)
    _check_chain(case, inp, pc, f"{cid} [producer / consumer]")
    for k in ("XT", "H1T", "H2T", "DZ2T", "DZ1T"):   # the critic workgroups run the same code in both forms
        assert np.array_equal(plain["raw"][k], pc["raw"][k]), f"{cid}: {k} differs between the two launch forms"
    assert np.array_equal(_bits(plain["Q"]), _bits(pc["Q"])), f"{cid}: Q differs between the two launch forms"


def test_chain_then_weight_gradient_agree_on_the_save_layout(ssa):
    """chain -> ssac_bf16_wgrad_lossfold (gradient mode) through the C entry points on the chain's own device buffers (Bp, the
    32-row rounding of XT, sentinel pad columns and all): the gradients are within the gradient-mode bound of the float64 reference
    evaluated from the device's saves"""
    cid = bc.CLOSING_CASE
    cc = bc._ALL[cid]
    cin = bc.chain_inputs(cc)
    got = run_chain(ssa, cc, cin, pc=False)
    n, i, nets = cc["n"], cc["in_dim"], cc["nets"]
    case = dict(cc, td="given", weight=1, popart=None, pop=0, denom=float(nets), only=None, id=cid + "-wgrad")
    g = bc._rng(case, "closing")
    w = lambda k: bc.bf16_widen(np.ascontiguousarray(got[k][:, :, :n])).reshape(nets, cc["H"], n).transpose(0, 2, 1).copy()
    inp = dict(kind="general", params=cin["critics"], X=bc.bf16_widen(np.ascontiguousarray(got["XT"][:i, :n])).reshape(i, n).T.copy(),
               H1=w("H1T"), H2=w("H2T"), DZ2=w("DZ2T"), DZ1=w("DZ1T"),
               lf=dict(gamma=np.float32(0.99), log_alpha=np.float32(0.0), Q=got["Q"].copy(), td=g.standard_normal(n).astype(np.float32),
                       weight=g.uniform(0.5, 1.5, n).astype(np.float32)))
    ref = bc.reference(case, inp)
    assert ref["flag_share"] < 0.01
    L = Wgrad(ssa, case, inp, "general", saves=got["raw"])
    _check_grads(L, L.run(), ref, "general", cid + " -> wgrad")
