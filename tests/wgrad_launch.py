"""The launch harness of the GPU tests of the fp32 weight-gradient launches (test_hip_wgrad_forms.py, test_hip_wgrad_fixed.py,
test_hip_wgrad_handoff.py): no tests of its own.

Launch         the device buffers of one wgrad_cases.py case and the launch of its entry point through the C ABI, every output
               followed by sentinel words; _check_grads / _check_lossfold compare what it wrote with the float64 references.
FixedLaunch    Launch of the `lossfold` entry in Adam mode with the log fold, the late-bound Polyak word and a misaligned arena:
               what the fixed-shape form of the merged launch (wgrad_fixed_kernel) is compared on, as BYTES against the general
               kernel (_same_bytes) and per element against float64 (_check_f64).
recorded_updates   whole critic updates at hidden 256, eager, then recorded and replayed.
switches_restored  puts back every form switch these tests turn.

Float64 in Adam mode runs on grid inputs, where the gradient is exact when denom * n_rows is a power of two IN FLOAT32 (the
kernels form it there); `_denom` picks denom = 2^k / n_rows and asserts that.  For 384, 160, 224 and 288 rows that denom is not
a float32 number: float32(denom) * n is 2^k only after the product's own rounding.  wgrad_cases.reference forms the product in
float64, a relative 2^-25 away -- nothing under ADAM_RTOL, except where the exact gradient is 0 and the float64 sum of the
rescaled terms is not.  `_reference` is wgrad_cases.reference with the row scale put back on the float32 product, which is the
kernels' formula (loss_fold_table); at 128 and 256 rows the two are the same numbers."""
import contextlib
import copy
import ctypes as C
import math
import random
from itertools import chain

import numpy as np
import torch

import synth
import wgrad_cases as wc

DEV = "cuda"
SENT, TAIL = wc.SENT, wc.TAIL
LOGW = 8            # floats of the test's log block: [0..2] loss / mean error / gradient norm, [4..6] the TD statistics
# everything a FixedLaunch writes (run_fold's result, where the mode has it)
BYTES = ("params", "m", "v", "target", "sumsq", "partials", "td_out", "logs", "td_stats", "tick", "done")
# Adam state of the launches that are compared with float64: zero moments, step 1 -- the step is then lr * sign(g) on integer
# parameters, so no element's new value cancels to nearly nothing (with seeded moments one element in ~10^5 does, and the 2 ulp +
# rtol bound of wgrad_cases.py is then tighter than float32 Adam itself, in the general kernel as in the fixed one).  Seeded
# moments are what the byte comparisons run on.
ADAM = dict(wd=0.0, target=1, seeded=0)


@contextlib.contextmanager
def switches_restored(ssa):
    """the library with every form switch these tests turn put back, whatever the body does"""
    lib = ssa._lib.lib
    try:
        yield lib
    finally:
        lib.ssac_wgrad_fixed(1)
        lib.ssac_wgrad_variant(0)
        lib.ssac_gemm_lean(1)
        lib.ssac_fused_tile_rows(0)


def _dev(a, lead=0):
    """device copy of a host array followed by TAIL sentinel words, `lead` floats off the allocation's (16-byte aligned) base"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.full((lead + a.size + TAIL,), SENT, device=DEV)
    buf[lead:lead + a.size] = torch.from_numpy(a).to(DEV)
    return buf, buf[lead:]


def _sent(numel):
    return torch.full((numel + TAIL,), SENT, device=DEV)


def _tail_ok(buf, numel, what):
    tail = torch.as_tensor(buf)[numel:numel + TAIL].cpu()
    assert torch.equal(tail, torch.full((TAIL,), SENT)), f"{what}: written past its end"


def _p(t):
    return 0 if t is None else t.data_ptr()


class Launch:
    """the device buffers of one (case, inputs) and the launch of its entry point"""

    def __init__(self, ssa, case, inp, adam=None):
        self.ssa, self.case, self.inp, self.adam = ssa, case, inp, adam
        c = case
        self.ids = wc.sel_ids(c)
        self.ns = len(self.ids)
        self.off, self.stride = wc.layout(c["in_dim"], c["H"], c["out"])
        offs = (C.c_int64 * 6)()
        assert ssa._lib.lib.ssac_mlp_layout(c["in_dim"], c["H"], c["out"], offs) == self.stride and list(offs) == self.off
        self.keep, self.pop = {}, None
        for k in ("H1", "H2", "DZ1", "DZ2", "DQ", "scale", "W3"):
            if k in inp:
                self.keep[k] = _dev(inp[k])[1]
        self.keep["Xbuf"], self.keep["X"] = _dev(inp["X"], lead=4 + c["xoff"])[0], None
        self.keep["X"] = self.keep["Xbuf"][4 + c["xoff"]:]
        assert (self.keep["X"].data_ptr() % 16 == 0) == (c["xoff"] == 0)
        self.ldx = wc.ldx_of(c)
        self.xs = c["n"] * self.ldx if c["x"] == "pernet" else 0
        self.ids_dev = torch.tensor(self.ids, dtype=torch.int32, device=DEV) if c["ids"] is not None else None
        self.tiles = [wc.wgrad_tiles(c, l) for l in range(3)]
        desc = ssa._lib.MlpDesc(0, self.stride, c["nets"], c["in_dim"], c["H"], c["out"])
        for l in range(3):
            want = ssa._lib.lib.ssac_head_wgrad_tiles(C.byref(desc)) if l == 2 and c["out"] <= 16 else None
            assert ssa._lib.lib.ssac_wgrad_tiles(C.byref(desc), l) == self.tiles[l] and want in (None, self.tiles[l])
        # a sumsq row: [head slots | GAP | fc2 slots | GAP | fc1 slots | GAP]
        # (none in the actor launch: its folded gradient norm sums the whole row of sumsq_net_stride slots)
        gap = 0 if c["entry"] == "actor" else wc.GAP
        self.ss_off = {2: 0, 1: self.tiles[2] + gap, 0: self.tiles[2] + self.tiles[1] + 2 * gap}
        self.ss_stride = sum(self.tiles) + 3 * gap
        if "lf" in inp:
            lf = inp["lf"]
            for k in ("Q", "td", "q_t", "logp", "rew", "done", "weight"):
                if k in lf:
                    self.keep[k] = _dev(lf[k])[1]
            self.keep["la"] = _dev(np.array([lf["log_alpha"]]))[1]
            pa = c["popart"]
            self.pop = ssa.engine.DeviceStruct(ssa._lib.PopArtState(0.3, 2.0, pa[0], pa[1], 5, 2, 1, 0, 1e-2), torch.device(DEV)) if pa else None
        if c["entry"] == "actor":
            g = wc._rng(c, "actor")
            self.a_parts = g.standard_normal(wc.ACTOR_TILES).astype(np.float32)
            self.keep["parts"] = _dev(self.a_parts)[1]

    def run(self, variant=0, lean=1, dz2_null=False):
        ssa, c, inp, k = self.ssa, self.case, self.inp, self.keep
        lib, st = ssa._lib.lib, ssa.engine.stream()
        ssa._lib.check(lib.ssac_wgrad_variant(variant))
        ssa._lib.check(lib.ssac_gemm_lean(lean))
        n, H, ns, nets = c["n"], c["H"], self.ns, c["nets"]
        total = nets * self.stride
        params_buf, params = _dev(inp["params"])
        out = dict(params=params_buf)
        ad = self.adam
        grads = m = v = tgt = ctl = None
        if ad is None:
            grads = out["grads"] = _sent(total)
        else:
            pad = np.full((nets, self.stride), SENT, np.float32)
            st_ = wc.adam_state(ad, (nets, self.stride))
            live = np.zeros((nets, self.stride), bool)
            live[:, :self.off[5] + c["out"]] = True
            arrs = [np.where(live, a, pad) for a in st_]
            m, v = out["m"], out["v"] = _dev(arrs[0])[0], _dev(arrs[1])[0]
            if ad["target"]:
                tgt = out["target"] = _dev(arrs[2])[0]
            f = wc.adam_ctl(ad)
            cs = ssa._lib.AdamCtl(f["lr"], f["beta1"], f["beta2"], f["eps"], f["wd"], f["step_size"], f["bc2_sqrt"], 1.0, f["step"],
                                  (C.c_int32 * 3)(0, 0, 0), wc.LR, wc.BETA1, wc.BETA2)
            ctl = self.ctl = ssa.engine.DeviceStruct(cs, torch.device(DEV))
        ss = out["sumsq"] = _sent(ns * self.ss_stride)
        ssp = lambda l: ss.data_ptr() + 4 * self.ss_off[l]
        desc = ssa._lib.MlpDesc(params.data_ptr(), self.stride, nets, c["in_dim"], H, c["out"])
        d, ids, X = C.byref(desc), _p(self.ids_dev), k["X"].data_ptr()
        mp, vp, cp, gp, tp = _p(m), _p(v), ctl.ptr if ctl else 0, _p(grads), _p(tgt)
        tau = wc.TAU if tgt is not None else 0.0
        e = c["entry"]
        if e == "fc12":
            rc = lib.ssac_mlp_wgrad_fc12(d, ids, ns, X, self.ldx, self.xs, _p(k["H1"]), _p(k["DZ2"]), _p(k["DZ1"]), n, mp, vp, cp, gp,
                                         ssp(1), ssp(0), self.ss_stride, tp, tau, st)
        elif e == "all":
            rc = lib.ssac_mlp_wgrad_all(d, ids, ns, X, self.ldx, self.xs, _p(k["H1"]), _p(k["H2"]), _p(k["DZ2"]), _p(k["DZ1"]),
                                        _p(k["DQ"]), n, mp, vp, cp, gp, ssp(2), ssp(1), ssp(0), self.ss_stride, tp, tau, st)
        elif e == "scaled":
            rc = lib.ssac_mlp_wgrad_all_scaled(d, ids, ns, X, self.ldx, self.xs, _p(k["H1"]), _p(k["H2"]), _p(k["DZ2"]), _p(k["DZ1"]),
                                               _p(k["scale"]), n, mp, vp, cp, gp, ssp(2), ssp(1), ssp(0), self.ss_stride, tp, tau, st)
        elif e == "lossfold":
            lf = inp["lf"]
            parts, td_out = out["partials"], out["td_out"] = _sent(2 * nets), _sent(n)
            spec = None
            if "q_t" in lf:
                spec = self.spec = ssa._lib.TdSpec(_p(k["q_t"]), _p(k["logp"]), _p(k["rew"]), _p(k["done"]), _p(k["la"]),
                                                   td_out.data_ptr(), float(lf["gamma"]), 2, 1, 0)
            rc = lib.ssac_mlp_wgrad_all_lossfold(
                d, X, self.ldx, self.xs, _p(k["H1"]), _p(k["H2"]), 0 if dz2_null else _p(k["DZ2"]), _p(k["DZ1"]), _p(k["W3"]),
                _p(k["Q"]), _p(k.get("td")), C.addressof(spec) if spec else 0, _p(k.get("weight")), self.pop.ptr if self.pop else 0,
                1 if self.pop else 0, float(c["denom"]), parts.data_ptr(), n, mp, vp, cp, gp, ssp(2), ssp(1), ssp(0),
                self.ss_stride, tp, tau, 0, st)
        elif e == "actor":
            done = out["done"] = torch.zeros(1 + TAIL, dtype=torch.int32, device=DEV)
            logs = out["logs"] = _dev(np.array([0.75, 0.0]))[0]
            fold = self.fold = ssa._lib.ActorLogFold(done.data_ptr(), _p(k["parts"]), wc.ACTOR_TILES, n, wc.ACTOR_INV, 0,
                                                     logs.data_ptr(), logs.data_ptr() + 4, 0, 0, 0)
            rc = lib.ssac_mlp_wgrad_all_actor(d, X, self.ldx, _p(k["H1"]), _p(k["H2"]), _p(k["DZ2"]), _p(k["DZ1"]), _p(k["DQ"]), n,
                                              mp, vp, cp, ssp(2), ssp(1), ssp(0), self.ss_stride, C.byref(fold), st)
        elif e.startswith("layer"):
            l = int(e[5])
            Xl, ld, xs = ((X, self.ldx, self.xs), (_p(k["H1"]), H, n * H), (_p(k["H2"]), H, n * H))[l]
            dY, w = ((k["DZ1"], H), (k["DZ2"], H), (k["DQ"], c["out"]))[l]
            rc = lib.ssac_mlp_layer_wgrad(d, l, ids, ns, Xl, ld, xs, _p(dY), w, n * w, n, mp, vp, cp, gp, ssp(l), self.ss_stride, tp,
                                          tau, st)
        else:
            assert e == "head"
            rc = lib.ssac_head_wgrad(d, ids, ns, _p(k["H2"]), _p(k["DQ"]), n, mp, vp, cp, gp, ssp(2), self.ss_stride, tp, tau, st)
        ssa._lib.check(rc)
        torch.cuda.synchronize()
        return {kk: vv.cpu().numpy() for kk, vv in out.items()}


    # ---- what the entry point writes
    def segs(self):
        e = self.case["entry"]
        if e == "fc12":
            return ("w1", "b1", "w2", "b2")
        if e == "head":
            return ("w3", "b3")
        if e.startswith("layer"):
            l = str(int(e[5]) + 1)
            return ("w" + l, "b" + l)
        return wc.SEGS

    def layers(self):
        return sorted({int(s[1]) - 1 for s in self.segs()})

    def seg_of(self, arena, slot, seg):
        sl = wc.seg_slices(self.case)[seg]
        return arena[:self.case["nets"] * self.stride].reshape(self.case["nets"], self.stride)[self.ids[slot], sl].reshape(
            wc.seg_shapes(self.case)[seg])

    def untouched_ok(self, arena, what, before=None):
        """every word of the arena outside the written segments of the selected nets: the sentinel (or the value before)"""
        nets = self.case["nets"]
        live = np.zeros((nets, self.stride), bool)
        for s in self.segs():
            live[self.ids, wc.seg_slices(self.case)[s]] = True
        a = arena[:nets * self.stride].reshape(nets, self.stride)
        want = np.full_like(a, SENT) if before is None else np.asarray(before, np.float32).reshape(nets, self.stride)
        assert np.array_equal(a[~live].view(np.uint32), want[~live].view(np.uint32)), f"{what}: words outside the launch's segments changed"
        assert np.array_equal(arena[nets * self.stride:], np.full(TAIL, SENT, np.float32)), f"{what}: written past its end"

    def sumsq_rows(self, ss):
        """per slot and layer the sum over the slots; gaps and tail must hold the sentinel"""
        rows = ss[:self.ns * self.ss_stride].reshape(self.ns, self.ss_stride)
        live = np.zeros(self.ss_stride, bool)
        sums = {}
        for l in self.layers():
            live[self.ss_off[l]:self.ss_off[l] + self.tiles[l]] = True
            sums[l] = rows[:, self.ss_off[l]:self.ss_off[l] + self.tiles[l]].astype(np.float64).sum(1)
        assert bool((rows[:, ~live] == SENT).all()) and bool((ss[self.ns * self.ss_stride:] == SENT).all()), "sumsq: written outside its slots"
        assert bool(np.isfinite(rows[:, live]).all()) and bool((rows[:, live] != SENT).all()), "sumsq: a slot of the launch was not written"
        return sums


def _check_grads(L, got, ref, kind, what):
    c = L.case
    L.untouched_ok(got["grads"], f"{what}: grads")
    assert np.array_equal(got["params"][:c["nets"] * L.stride], L.inp["params"].reshape(-1)), f"{what}: gradient store changed the parameters"
    sums = L.sumsq_rows(got["sumsq"])
    for slot in range(L.ns):
        g2 = {l: 0.0 for l in L.layers()}
        tol = {l: 0.0 for l in L.layers()}
        for s in L.segs():
            g, S = ref[s][0][slot], ref[s][1][slot]
            have = L.seg_of(got["grads"], slot, s).astype(np.float64)
            d = np.zeros_like(g) if kind == "grid" else wc.bound(s, S)
            if kind == "grid":
                assert np.array_equal(have, g.reshape(have.shape)), \
                    f"{what}: {s} of slot {slot} (net {L.ids[slot]}) differs from the exact sums in {int((have != g.reshape(have.shape)).sum())} elements"
            else:
                ratio = np.abs(have - g.reshape(have.shape)) / np.maximum(d.reshape(have.shape), 1e-300)
                assert float(ratio.max()) <= 1.0, f"{what}: {s} of slot {slot} (net {L.ids[slot]}) off by {float(ratio.max()):.3g} bounds"
            g2[int(s[1]) - 1] += float((g * g).sum())
            tol[int(s[1]) - 1] += wc.sumsq_tol(g, d)
        # per net over ALL slots of the launch: the head workgroups that own fc2's bias gradient (with_b2) add its square to
        # the head's slots, so only the per-net total is defined
        have2, want2 = sum(sums[l][slot] for l in L.layers()), sum(g2.values())
        assert abs(have2 - want2) <= sum(tol.values()), f"{what}: sumsq of slot {slot}: {have2!r} vs {want2!r}"


def _check_lossfold(L, got, kind, what):
    c, inp = L.case, L.inp
    s = wc.loss_scale(c, inp)
    _tail_ok(got["partials"], 2 * c["nets"], "partials")
    _tail_ok(got["td_out"], c["n"], "td_out")
    parts = got["partials"][:2 * c["nets"]].reshape(c["nets"], 2).astype(np.float64)
    for e in range(c["nets"]):
        for j, terms in ((0, s["werr2"][e]), (1, s["err"][e])):
            if kind == "grid":
                assert parts[e, j] == terms.sum(), f"{what}: partials[{e}][{j}] on the grid"
            assert abs(parts[e, j] - terms.sum()) / c["n"] <= wc.log_tol(terms), f"{what}: partials[{e}][{j}] {parts[e, j]!r} vs {terms.sum()!r}"
    if "q_t" in inp["lf"]:
        td = got["td_out"][:c["n"]].astype(np.float64)
        assert bool((np.abs(td - s["td"]) <= (0.0 if kind == "grid" else wc.td_tol(inp["lf"]))).all()), f"{what}: td_out"
    else:
        assert bool((got["td_out"] == SENT).all()), f"{what}: td_out written though td was given"


# ---- the `lossfold` entry in Adam mode: what the fixed-shape form is compared on ------------------------------------------

def _denom(n):
    """denom with float32(denom) * float32(n) a power of two in float32 (module docstring)"""
    d = 2.0 ** math.ceil(math.log2(n)) / n
    p2 = float(np.float32(d) * np.float32(n))
    assert p2 == 2.0 ** round(math.log2(p2))
    return d


def _case(n, nets=1, in_dim=23, H=256, out=1, entry="lossfold", **kw):
    kw.setdefault("denom", _denom(n))
    kw.setdefault("td", "lazy")
    c = wc._c(entry, n, in_dim=in_dim, H=H, out=out, nets=nets, **kw)
    c["id"] = "fixed-" + "-".join(f"{k}{wc._fmt(k, v)}" for k, v in sorted(c.items()) if k != "entry") + "-" + entry
    return c


_INPUTS = {}


def _p2(case):
    """denom * n_rows as the kernels form it: one float32 product"""
    return float(np.float32(case["denom"]) * np.float32(case["n"]))


def _reference(case, inp):
    """wgrad_cases.reference of a `lossfold` case with dL/dq scaled by 1 / (denom * n) on the FLOAT32 product (module docstring)"""
    pw = np.float64(np.float32(case["popart"][0])) if case["popart"] else np.float64(1.0)
    w = inp["lf"]["weight"].astype(np.float64) if "weight" in inp["lf"] else np.ones(case["n"])
    scale = ((np.float64(-2.0) * pw / _p2(case)) * w[None, :] * wc.loss_scale(case, inp)["err"])[wc.sel_ids(case)]
    out = {}
    for l, (A, B) in wc.operands(case, inp, scale=scale).items():
        Bb = np.broadcast_to(B, (A.shape[0],) + B.shape[1:])
        out["w" + l] = (np.einsum("ekm,ekn->emn", A, Bb), np.einsum("ekm,ekn->emn", np.abs(A), np.abs(Bb)))
        out["b" + l] = (A.sum(1), np.abs(A).sum(1))
    return out


def _inputs(case):
    """grid inputs and the float64 reference of a case: drawn once, shared, read-only"""
    if case["id"] not in _INPUTS:
        inp = wc.make_inputs(case, "grid")
        _INPUTS[case["id"]] = (inp, _reference(case, inp) if case["entry"] == "lossfold" else wc.reference(case, inp))
    return _INPUTS[case["id"]]


class FixedLaunch(Launch):
    """Launch of the `lossfold` entry in Adam mode with what Launch leaves at NULL: the log fold (folded or deferred), the
    late-bound Polyak word, and arenas 4 bytes off a 16-byte boundary.  No gaps between the layers' slots of a sumsq row: the
    folded gradient norm sums the whole row."""

    def __init__(self, ssa, case, inp, adam):
        super().__init__(ssa, case, inp, adam=adam)
        self.ss_off = {2: 0, 1: self.tiles[2], 0: self.tiles[2] + self.tiles[1]}
        self.ss_stride = sum(self.tiles)

    def run_fold(self, fixed, dz2_null=False, late=None, logs="none", lead=0, grads=False):
        """late: None = static tau, else the float the late word holds (0.0 = no soft update followed)"""
        ssa, c, inp, k = self.ssa, self.case, self.inp, self.keep
        lib, st = ssa._lib.lib, ssa.engine.stream()
        ssa._lib.check(lib.ssac_wgrad_variant(1))
        ssa._lib.check(lib.ssac_wgrad_fixed(1 if fixed else 0))
        n, nets, ad = c["n"], c["nets"], self.adam
        total = nets * self.stride
        out = {}
        out["params"], params = _dev(inp["params"], lead=lead)
        m = v = tgt = g = None
        if grads:
            g = out["grads"] = _sent(total)
        else:
            st_ = wc.adam_state(ad, (nets, self.stride))
            live = np.zeros((nets, self.stride), bool)
            live[:, :self.off[5] + c["out"]] = True
            arrs = [np.where(live, a, np.float32(SENT)) for a in st_]
            (out["m"], m), (out["v"], v) = _dev(arrs[0], lead=lead), _dev(arrs[1], lead=lead)
            if ad["target"]:
                out["target"], tgt = _dev(arrs[2], lead=lead)
        f = wc.adam_ctl(ad)
        cs = ssa._lib.AdamCtl(f["lr"], f["beta1"], f["beta2"], f["eps"], f["wd"], f["step_size"], f["bc2_sqrt"], 1.0, f["step"],
                              (C.c_int32 * 3)(0, 0, 0), wc.LR, wc.BETA1, wc.BETA2)
        self.ctl = ssa.engine.DeviceStruct(cs, torch.device(DEV))
        ss = out["sumsq"] = _sent(self.ns * self.ss_stride)
        ssp = lambda l: ss.data_ptr() + 4 * self.ss_off[l]
        desc = ssa._lib.MlpDesc(params.data_ptr(), self.stride, nets, c["in_dim"], c["H"], c["out"])
        lf = inp["lf"]
        parts, td_out = out["partials"], out["td_out"] = _sent(2 * nets), _sent(n)
        spec = None
        if "q_t" in lf:
            spec = self.spec = ssa._lib.TdSpec(_p(k["q_t"]), _p(k["logp"]), _p(k["rew"]), _p(k["done"]), _p(k["la"]),
                                               td_out.data_ptr(), float(lf["gamma"]), 2, 1, 0)
        word = feed = None
        if late is not None:
            word = self.word = torch.from_numpy(np.array([late, 0, 0, 0], np.float32)).to(DEV)
        fold = None
        if logs == "folded":
            done = out["done"] = torch.zeros(1 + TAIL, dtype=torch.int32, device=DEV)
            blk = out["logs"] = _dev(np.array([0.75] + [0.0] * (LOGW - 1), np.float32))[0]
            fold = ssa._lib.LogFold(done.data_ptr(), blk.data_ptr(), blk.data_ptr() + 16 if spec else 0, 0, 0, _p(word))
        elif logs == "deferred":
            assert spec is not None
            feed = self.feed = ssa.engine.DeviceStruct(ssa._lib.Feed(0, 0, 0, 41, 4, 0, 0, LOGW, 0), torch.device(DEV))
            stats = out["td_stats"] = _sent(3)
            fold = ssa._lib.LogFold(0, 0, 0, feed.ptr, stats.data_ptr(), _p(word))
        elif word is not None:
            fold = ssa._lib.LogFold(0, 0, 0, 0, 0, word.data_ptr())
        self.fold = fold
        rc = lib.ssac_mlp_wgrad_all_lossfold(
            C.byref(desc), k["X"].data_ptr(), self.ldx, self.xs, _p(k["H1"]), _p(k["H2"]), 0 if dz2_null else _p(k["DZ2"]),
            _p(k["DZ1"]), _p(k["W3"]), _p(k["Q"]), _p(k.get("td")), C.addressof(spec) if spec else 0, _p(k.get("weight")),
            self.pop.ptr if self.pop else 0, 1 if self.pop else 0, float(c["denom"]), parts.data_ptr(), n, _p(m), _p(v),
            0 if grads else self.ctl.ptr, _p(g), ssp(2), ssp(1), ssp(0), self.ss_stride, _p(tgt), wc.TAU if tgt is not None else 0.0,
            C.byref(fold) if fold else 0, st)
        ssa._lib.check(rc)
        torch.cuda.synchronize()
        got = {kk: vv.cpu().numpy()[lead:] if kk in ("params", "m", "v", "target") else vv.cpu().numpy() for kk, vv in out.items()}
        if feed is not None:
            got["tick"] = np.array([feed.read().tick], np.int64)
        got["taken"] = lib.ssac_wgrad_fixed_taken()
        return got


def _same_bytes(a, b, what):
    assert set(a) == set(b)
    for k in BYTES:
        if k in a:
            assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs between the fixed and the general form"


def _check_f64(L, got, ref, what, late=None, logs="none"):
    """test_hip_wgrad_forms.test_adam_and_polyak_epilogues' comparison: m, v, p [, target] per element against a float64 Adam on
    the float64 gradient, the per-net sumsq total, the loss partials and td_out; then the logs"""
    case, inp, ad = L.case, L.inp, L.adam
    ctl = wc.adam_ctl(ad)
    nets = case["nets"]
    old = dict(zip(("m", "v", "target"), wc.adam_state(ad, (nets, L.stride))), p=inp["params"])
    got = dict(got, p=got["params"])
    polyak = bool(ad["target"]) and (late is None or late != 0.0)
    tau = wc.TAU if late is None else late
    keys = ("m", "v", "p") + (("target",) if ad["target"] else ())
    for k in keys:
        before = old[k].copy()
        before[:, L.off[5] + case["out"]:] = SENT
        L.untouched_ok(got[k], f"{what}: {k}", before=before)
    sums = L.sumsq_rows(got["sumsq"])
    g2tot = 0.0
    for slot in range(L.ns):
        g2 = 0.0
        for s in L.segs():
            g = ref[s][0][slot]
            sl = wc.seg_slices(case)[s]
            o = {k: old[k][L.ids[slot], sl].reshape(g.shape) for k in ("m", "v", "p", "target")}
            r = wc.adam_ref(ctl, o["p"], g, o["m"], o["v"], o["target"] if ad["target"] else None)
            if ad["target"]:   # (adam_ref applies wc.TAU: the late-bound word may hold another tau, or none)
                r["target"] = o["target"].astype(np.float64) * (1.0 - np.float64(np.float32(tau))) + r["p"] * np.float64(np.float32(tau)) \
                    if polyak else o["target"].astype(np.float64)
            for k in keys:
                have = L.seg_of(got[k], slot, s).astype(np.float64).reshape(g.shape)
                if k == "target" and not polyak:
                    assert np.array_equal(have, r[k]), f"{what}: the target moved though no soft update was asked for"
                    continue
                bad = np.abs(have - r[k]) > wc.adam_tol(o[k], r[k])
                assert not bad.any(), f"{what}: {k} of {s}, slot {slot}: {int(bad.sum())} of {bad.size} off"
            g2 += float((g * g).sum())
        have2 = sum(sums[l][slot] for l in L.layers())
        assert abs(have2 - g2) <= 1e-5 * g2, f"{what}: sumsq of slot {slot}: {have2!r} vs {g2!r}"
        g2tot += g2
    _check_lossfold(L, got, "grid", what)
    s = wc.loss_scale(case, inp)
    td = s["td"]
    stats = (td.mean(), td.std(ddof=1), (math.exp(float(inp["lf"]["log_alpha"])) * inp["lf"]["logp"].astype(np.float64)).mean()) \
        if "q_t" in inp["lf"] else None
    if logs == "folded":
        lg = got["logs"].astype(np.float64)
        n = case["n"]
        want0 = 0.75 + s["werr2"].sum() / _p2(case)
        assert abs(lg[0] - want0) <= wc.log_tol(s["werr2"]) * nets + 1e-6, f"{what}: folded loss {lg[0]!r} vs {want0!r}"
        assert abs(lg[1] - s["err"][nets - 1].mean()) <= wc.log_tol(s["err"][nets - 1]), f"{what}: folded mean error"
        assert abs(lg[2] - math.sqrt(g2tot)) <= 1e-5 * math.sqrt(g2tot), f"{what}: folded gradient norm"
        if stats:
            for j, want in enumerate(stats):
                assert abs(lg[4 + j] - want) <= 1e-5 * abs(want) + wc.log_tol(td), f"{what}: folded TD statistic {j}"
        assert bool((got["logs"][LOGW:] == SENT).all()) and int(got["done"][0]) == 0 and not got["done"][1:].any(), f"{what}: log block / counter"
    if logs == "deferred":
        for j, want in enumerate(stats):
            assert abs(float(got["td_stats"][j]) - want) <= 1e-5 * abs(want) + wc.log_tol(td), f"{what}: deferred TD statistic {j}"
        assert bool((got["td_stats"][3:] == SENT).all()) and int(got["tick"][0]) == 42, f"{what}: deferred stats / the ring's tick"


# ---- whole recorded updates ------------------------------------------------------------------------------------------------

def recorded_updates(ssa, *, fixed, B, N, pop, weights, n_upd, tile_rows=None, every_update=False):
    """n_upd critic updates at hidden 256 with the 64 x 64 weight-gradient form forced (and `tile_rows`-row critic tiles, if
    given) -- eager, then recorded and replayed: chained launch, weight-gradient launch with Adam, Polyak every second update.
    ssac_wgrad_fixed(fixed) throughout.  Returns (snapshots, taken).  A snapshot holds parameters, targets, both moments and the
    logs of every update so far; with every_update there is one after EVERY update, with that update's TD targets beside them,
    else one after the last.  taken[k]: the form the weight-gradient launch of update k took (a replayed update issues no
    launcher call: it repeats the form of the launch that was recorded)."""
    L, lib = ssa.learning, ssa._lib.lib
    dev = torch.device("cuda")
    S, A, H = 17, 6, 256
    ssa._lib.check(lib.ssac_wgrad_fixed(1 if fixed else 0))
    ssa._lib.check(lib.ssac_fused_tile_rows(tile_rows or 0))
    ssa._lib.check(lib.ssac_wgrad_variant(1))
    assert L.USE_GRAPHS and L.LAUNCH_MODE == "list"
    torch.manual_seed(3); np.random.seed(3); random.seed(3)
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(S),
                      actor_network_cls=ssa.nets.ContinuousStochasticActor,
                      critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=N,
                      hidden_size=H, auto_rescale_targets=pop, log_std_low=-5.0, log_std_high=2.0)
    agent.to(dev)
    target = copy.deepcopy(agent)
    buf = ssa.replay.ReplayBuffer(4096, device=dev)
    buf.load_experience(*synth.synth_transitions(2000, S, A, seed=5))
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4)
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    la = torch.Tensor([math.log(0.1)]).to(dev); la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    flat = lambda mods: torch.cat([p.detach().flatten() for m in mods for p in m.parameters()]).cpu().numpy()

    def snapshot(**more):
        m, v = copt._ssac_adam.moments_for(("critic", 0), agent.critics[0].arena(dev).params)
        return dict(params=flat(agent.critics), target=flat(target.critics), m=m.detach().cpu().numpy().copy(),
                    v=v.detach().cpu().numpy().copy(), logs=np.array(logs, np.float64), **more)

    snapshots, taken, logs = [], [], []
    for k in range(n_upd):
        res = L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
            log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
            target_critic_ensemble_n=2, weighted_bellman_temp=10.0 if weights else None,
            weight_type="sunrise" if weights else None, pop=pop, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
            discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
        lg, dicts = res if isinstance(res, tuple) else (res, None)
        logs.append([float(v_) for _, v_ in sorted(dict(lg).items())])   # (read now: the values are views of a ring slot)
        taken.append(lib.ssac_wgrad_fixed_taken())
        td = dicts[0]["td_target"].detach().cpu().numpy().copy() if every_update else None
        if k % 2 == 0:
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
        if every_update:
            snapshots.append(snapshot(td=td))
    torch.cuda.synchronize()
    if not every_update:
        snapshots.append(snapshot())
    return snapshots, taken

