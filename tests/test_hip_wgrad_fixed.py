"""GPU: the fixed-shape form of the merged weight-gradient launch (wgrad_fixed_kernel, csrc/ssac_gemm.hip) against the general
lean kernel it stands in for, and both against float64.

The fixed form leaves every floating-point operation and its order alone, so a launch with ssac_wgrad_fixed(1) and with (0) is
compared as BYTES over everything it writes: parameters, both moments, the target arena, the gradient-norm slots, the loss
partials, td_out and the logs (folded) or the TD statistics and the ring's tick (deferred).  Inputs, layouts, float64 references
and tolerances are those of wgrad_cases.py (the `lossfold` entry in Adam mode); the launch harness is test_hip_wgrad_forms.Launch
with the log fold, the late-bound Polyak and a misaligned arena added.

Small launches take the 32 x 32 latency form by themselves: the 64 x 64 form is forced (ssac_wgrad_variant(1)).

Rows.  The fixed form is the lean kernel with FOUR K-groups, and the launcher gives a launch four K-groups from 8 chunks of 32
rows on (wgrad_merged: 2 below that), so 256 rows -- two iterations per K-group -- is the smallest launch that takes it and
384 the smallest with an odd iteration count.  At 128 rows (one chunk per K-group if there were four) the launch has two
K-groups and keeps the general kernel; the row ladder keeps that size and pins it as declined.  288 rows (nine chunks over four
groups) is the size at which the lean loader itself declines.

Weight decay, PopArt and per-row weights travel in the Adam control block and in the loss fold's arguments, which both forms
read alike: such launches TAKE the fixed form, with equal bits (test_decay_popart_and_weights_take_the_fixed_form).

Float64.  Adam mode runs on grid inputs, where the gradient is exact when denom * n_rows is a power of two IN FLOAT32 (the
kernels form it there); `_denom` picks denom = 2^k / n_rows and asserts that.  For 384, 160, 224 and 288 rows that denom is not
a float32 number: float32(denom) * n is 2^k only after the product's own rounding.  wgrad_cases.reference forms the product in
float64, a relative 2^-25 away -- nothing under ADAM_RTOL, except where the exact gradient is 0 and the float64 sum of the
rescaled terms is not.  `_reference` is wgrad_cases.reference with the row scale put back on the float32 product, which is the
kernels' formula (loss_fold_table); at 128 and 256 rows the two are the same numbers.
"""
import ctypes as C
import copy
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import synth
import wgrad_cases as wc
from test_hip_wgrad_forms import Launch, _check_grads, _check_lossfold, _dev, _p, _sent

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT, TAIL = wc.SENT, wc.TAIL
LOGW = 8            # floats of the test's log block: [0..2] loss / mean error / gradient norm, [4..6] the TD statistics
BYTES = ("params", "m", "v", "target", "sumsq", "partials", "td_out", "logs", "td_stats", "tick", "done")


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


@pytest.fixture(autouse=True)
def _switches_restored(ssa):
    lib = ssa._lib.lib
    try:
        yield
    finally:
        lib.ssac_wgrad_fixed(1)
        lib.ssac_wgrad_variant(0)
        lib.ssac_gemm_lean(1)


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
    """Launch of the `lossfold` entry in Adam mode with what test_hip_wgrad_forms.Launch leaves at NULL: the log fold (folded or
    deferred), the late-bound Polyak word, and arenas 4 bytes off a 16-byte boundary.  No gaps between the layers' slots of a
    sumsq row: the folded gradient norm sums the whole row."""

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


# Adam state of the launches that are compared with float64: zero moments, step 1 -- the step is then lr * sign(g) on integer
# parameters, so no element's new value cancels to nearly nothing (with seeded moments one element in ~10^5 does, and the 2 ulp +
# rtol bound of wgrad_cases.py is then tighter than float32 Adam itself, in the general kernel as in the fixed one).  Seeded
# moments are what the byte comparison's extra mode runs on.
ADAM = dict(wd=0.0, target=1, seeded=0)
# (rows, nets, in_dim): the row ladder at the headline's width, the nets (per-class XCD mixing on only at N = 2: the class counts
# 16 N, 4 N, 4 N are multiples of 8 there), the input widths 4 / 23 (ragged last vector of the x rows) / 32 (a full block)
SHAPES = [(128, 1, 23), (256, 1, 23), (384, 1, 23), (256, 2, 23), (256, 3, 23), (256, 1, 4), (384, 2, 32)]
# (dz2u rebuilt, late word (None: static tau), target arena, logs, seeded moments: bytes only)
MODES = [(False, None, 1, "none", 0), (True, None, 1, "folded", 0), (False, wc.TAU, 1, "deferred", 0), (True, 0.0, 1, "folded", 0),
         (False, None, 0, "deferred", 0), (True, 0.125, 1, "none", 0), (True, wc.TAU, 1, "folded", 1)]


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


def _recorded_updates(ssa, fixed, B=256, N=2, pop=False, weights=False, n_upd=6):
    """critic updates at hidden 256 with the 64 x 64 weight-gradient form forced -- eager, then recorded and replayed: chained
    launch, weight-gradient launch with Adam, Polyak every second update.  Returns parameters, targets, moments and every
    update's logs, and the form the last weight-gradient launch took after every update."""
    L, lib = ssa.learning, ssa._lib.lib
    dev = torch.device("cuda")
    S, A, H = 17, 6, 256
    ssa._lib.check(lib.ssac_wgrad_fixed(1 if fixed else 0))
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
    taken, logs = [], []
    for k in range(n_upd):
        lg = L.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt,
            log_alphas=[la], batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None,
            target_critic_ensemble_n=2, weighted_bellman_temp=10.0 if weights else None,
            weight_type="sunrise" if weights else None, pop=pop, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
            discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
        lg = lg[0] if isinstance(lg, tuple) else lg
        logs.append({k_: float(v_) for k_, v_ in dict(lg).items()})   # (read now: the values are views of a ring slot)
        taken.append(lib.ssac_wgrad_fixed_taken())
        if k % 2 == 0:
            ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], 0.005)
    torch.cuda.synchronize()
    flat = lambda mods: torch.cat([p.detach().flatten() for m in mods for p in m.parameters()]).cpu().numpy()
    ar = agent.critics[0].arena(dev)
    m, v = copt._ssac_adam.moments_for(("critic", 0), ar.params)
    logv = np.array([[float(v_) for _, v_ in sorted(dict(lg).items())] for lg in logs], np.float64)
    return dict(params=flat(agent.critics), target=flat(target.critics), m=m.detach().cpu().numpy().copy(),
                v=v.detach().cpu().numpy().copy(), logs=logv), taken


@pytest.mark.parametrize("setting", ["plain", "popart", "per-row weights"])
def test_recorded_update_ends_on_the_same_bits_with_either_form(ssa, setting):
    """Whole updates -- eager, recorded and replayed, Polyak every second -- with the switch on and off: final arenas, moments,
    targets and every update's logs equal as bytes.  B 256 / N 2: the smallest batch whose weight-gradient launch has four
    K-groups (module docstring).  PopArt needs the target Q in one part, which the engine forms at the benchmark's shape only."""
    kw = dict(pop=setting == "popart", weights=setting == "per-row weights")
    if setting == "popart":
        kw.update(B=512, N=10)
    a, taken_a = _recorded_updates(ssa, True, **kw)
    b, taken_b = _recorded_updates(ssa, False, **kw)
    print(setting, "weight-gradient launches took (switch on):", taken_a, "(off):", taken_b)
    assert all(t == 0 for t in taken_b)
    if setting == "plain":
        assert all(t == 1 for t in taken_a)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{setting}: {k} differs between the fixed and the general form"
    assert np.isfinite(a["params"]).all() and float(np.abs(a["m"]).max()) > 0
