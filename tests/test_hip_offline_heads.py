"""GPU: the offline-update and weighting row kernels (ssac_adv_filter, ssac_adv_filter_discrete, ssac_bc_logprob_bwd,
ssac_bc_discrete_bwd, ssac_bc_det_logprob_bwd, ssac_action_invariance_det_bwd, ssac_actor_loss_bwd_adv, ssac_dr3_add,
ssac_softmax_weights, ssac_sunrise_weights, ssac_ensemble_min_select) through the C ABI, every output element and every log
word against the float64 references of offline_head_cases.py, at row counts around the wave (64) and workgroup (1024)
boundaries of their single-workgroup row loops.  Inputs, references and tolerances: offline_head_cases.py; every output is
followed by sentinel words that must survive, padding columns of strided outputs likewise."""
import pytest
import torch

import offline_head_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _buf(numel, head=None):
    """numel words (head, or sentinels) followed by TAIL sentinel words"""
    b = torch.full((numel + oc.TAIL,), oc.SENT, device=DEV)
    if head is not None:
        b[:numel] = torch.as_tensor(head, dtype=torch.float32).reshape(-1).to(DEV)
    return b


def _tail_ok(buf, numel, what):
    assert torch.equal(buf[numel:].cpu(), torch.full((oc.TAIL,), oc.SENT)), f"{what}: written past its end"


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _dev(t):
    return t.to(DEV) if t is not None else None


def _popart(ssa, wb):
    if wb is None:
        return None
    return ssa.engine.DeviceStruct(ssa._lib.PopArtState(0.3, 2.0, wb[0], wb[1], 5, 2, 1, 0, 1e-2), torch.device(DEV))


def _close(got, ref, family, what):
    got, ref = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1)
    rt, at = oc.rtol(family), oc.atol_of(ref)
    print(f"{what}: deviation {oc.rel_dev(got, ref):.3g} (rtol {rt:.3g}), max |diff| {float((got - ref).abs().max()):.3g} (atol {at:.3g})")
    bad = ((got - ref).abs() > at + rt * ref.abs()).nonzero().reshape(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {ref.numel()} off, first at {int(bad[0])}: {float(got[bad[0]])} vs {float(ref[bad[0]])}"


def _word(got, ref, tol, what):
    got, ref = float(got), float(ref)
    print(f"{what}: {got!r} vs {ref!r}, |diff| {abs(got - ref):.3g} (tol {tol:.3g})")
    assert abs(got - ref) <= tol, what


def _exact(got, ref, what):
    assert torch.equal(got.detach().cpu(), ref.float()), what


def _filter_checks(case, ref, outs, logs):
    n = case["n"]
    for k, b in outs.items():
        _tail_ok(b, n, k)
    _tail_ok(logs, 1, "logs")
    if "mask" in outs:
        _exact(outs["mask"][:n], ref["mask"], "mask")
    if "adv" in outs:
        if case["exact"]:
            _exact(outs["adv"][:n], ref["adv"], "adv on the grid")
        else:
            _close(outs["adv"][:n], ref["adv"], case["family"], "adv")
    if "prio" in outs:
        _close(outs["prio"][:n], ref["prio"], case["family"], "prio")
    if case["exact"]:   # the planted rows: advantage exactly 0 passes the filter and takes the floor priority
        rows = oc._planted(n)
        assert float(ref["adv"][rows].abs().max()) == 0.0
        if "mask" in outs:
            assert bool((outs["mask"][rows] == 1.0).all())
        if "prio" in outs:
            _exact(outs["prio"][rows], torch.full((len(rows),), 1e-4), "floor priority")
    _word(logs[0], ref["logs"], oc.log_tol(ref["terms"]), "mean(mask)")


@pytest.mark.parametrize("cid", oc.ids("adv_filter"))
def test_adv_filter(ssa, cid):
    case, inp, ref = oc.load("adv_filter", cid)
    n = case["n"]
    q, pop = inp["q"].to(DEV), _popart(ssa, case["popart"])
    outs = {k: _buf(n) for k in ("adv", "mask", "prio") if case["null"] != k}
    logs = _buf(1)
    ssa._lib.check(ssa._lib.lib.ssac_adv_filter(
        q.data_ptr(), case["nets"], n, case["samp"], pop.ptr if pop else 0, case["max"], _ptr(outs.get("adv")),
        _ptr(outs.get("mask")), _ptr(outs.get("prio")), logs.data_ptr(), ssa.engine.stream()))
    _filter_checks(case, ref, outs, logs)


@pytest.mark.parametrize("cid", oc.ids("adv_filter_discrete"))
def test_adv_filter_discrete(ssa, cid):
    case, inp, ref = oc.load("adv_filter_discrete", cid)
    n = case["n"]
    q, logits, act, pop = inp["q"].to(DEV), inp["logits"].to(DEV), inp["act"].to(DEV), _popart(ssa, case["popart"])
    outs = {k: _buf(n) for k in ("adv", "mask", "prio") if case["null"] != k}
    logs = _buf(1)
    ssa._lib.check(ssa._lib.lib.ssac_adv_filter_discrete(
        q.data_ptr(), case["nets"], n, case["A"], logits.data_ptr(), case["actors"], act.data_ptr(), case["ld"],
        pop.ptr if pop else 0, _ptr(outs.get("adv")), _ptr(outs.get("mask")), _ptr(outs.get("prio")), logs.data_ptr(),
        ssa.engine.stream()))
    _filter_checks(case, ref, outs, logs)


def _bc_checks(case, ref, d, ld_dout, width, member, total):
    """the gradient block (n x ld_dout, the first `width` columns written), the member's loss word and the accumulated one"""
    n = case["n"]
    _tail_ok(d, n * ld_dout, "d_out")
    dd = d[:n * ld_dout].view(n, ld_dout).cpu()
    assert torch.equal(dd[:, width:], torch.full((n, ld_dout - width), oc.SENT)), "padding columns of d_out written"
    _tail_ok(total, 1, "logs_total")
    if member is not None:
        _tail_ok(member, 1, "logs_member")
    if case["mask"] == "zero":   # nothing passes the filter: no gradient, no loss, the accumulated word unchanged
        assert bool((dd[:, :width] == 0.0).all()) and float(total[0]) == oc.PRE
        assert member is None or float(member[0]) == 0.0
        return
    _close(dd[:, :width], ref["d_out"], case["family"], "d_out")
    if member is not None:
        _word(member[0], ref["member"], oc.log_tol(ref["terms"]), "logs_member")
    _word(total[0], ref["total"], oc.log_tol(ref["terms"] * case["inv"]), "logs_total")


@pytest.mark.parametrize("cid", oc.ids("bc_logprob"))
def test_bc_logprob_bwd(ssa, cid):
    case, inp, ref = oc.load("bc_logprob", cid)
    n, A = case["n"], case["A"]
    ld_out, ld_act, ld_dout = oc.bc_strides(case, 2 * A)
    out, act, mask = inp["out"].to(DEV), inp["act"].to(DEV), _dev(inp["mask"])
    d, member, total = _buf(n * ld_dout), _buf(1) if case["member"] else None, _buf(1, [oc.PRE])
    ssa._lib.check(ssa._lib.lib.ssac_bc_logprob_bwd(
        out.data_ptr(), ld_out, act.data_ptr(), ld_act, _ptr(mask), n, A, case["lo"], oc.BC_HI, case["inv"], d.data_ptr(),
        ld_dout, _ptr(member), total.data_ptr(), ssa.engine.stream()))
    _bc_checks(case, ref, d, ld_dout, 2 * A, member, total)


@pytest.mark.parametrize("cid", oc.ids("bc_discrete"))
def test_bc_discrete_bwd(ssa, cid):
    case, inp, ref = oc.load("bc_discrete", cid)
    n, A = case["n"], case["A"]
    logits, act, mask = inp["logits"].to(DEV), inp["act"].to(DEV), _dev(inp["mask"])
    d, member, total = _buf(n * A), _buf(1) if case["member"] else None, _buf(1, [oc.PRE])
    ssa._lib.check(ssa._lib.lib.ssac_bc_discrete_bwd(
        logits.data_ptr(), act.data_ptr(), act.shape[1], _ptr(mask), n, A, case["inv"], d.data_ptr(), _ptr(member),
        total.data_ptr(), ssa.engine.stream()))
    _bc_checks(case, ref, d, A, A, member, total)


@pytest.mark.parametrize("cid", oc.ids("bc_det"))
def test_bc_det_logprob_bwd(ssa, cid):
    case, inp, ref = oc.load("bc_det", cid)
    n, A = case["n"], case["A"]
    ld_out, ld_act, ld_dout = oc.bc_strides(case, A)
    out, act, mask = inp["out"].to(DEV), inp["act"].to(DEV), _dev(inp["mask"])
    d, member, total = _buf(n * ld_dout), _buf(1) if case["member"] else None, _buf(1, [oc.PRE])
    ssa._lib.check(ssa._lib.lib.ssac_bc_det_logprob_bwd(
        out.data_ptr(), ld_out, act.data_ptr(), ld_act, _ptr(mask), n, A, case["inv"], d.data_ptr(), ld_dout, _ptr(member),
        total.data_ptr(), ssa.engine.stream()))
    _bc_checks(case, ref, d, ld_dout, A, member, total)


@pytest.mark.parametrize("cid", oc.ids("actinv_det"))
def test_action_invariance_det_bwd(ssa, cid):
    case, inp, ref = oc.load("actinv_det", cid)
    n, A = case["n"], case["A"]
    ld_o, ld_a, ld_dout = oc.bc_strides(case, A)
    out_o, out_a = inp["out_o"].to(DEV), inp["out_a"].to(DEV)
    d, loss, total = _buf(n * ld_dout), _buf(1), _buf(1, [oc.PRE]) if case["add"] else None
    ssa._lib.check(ssa._lib.lib.ssac_action_invariance_det_bwd(
        out_o.data_ptr(), ld_o, out_a.data_ptr(), ld_a, n, A, case["coeff"], d.data_ptr(), ld_dout, loss.data_ptr(),
        _ptr(total), ssa.engine.stream()))
    _tail_ok(d, n * ld_dout, "d_out")
    _tail_ok(loss, 1, "loss_out")
    dd = d[:n * ld_dout].view(n, ld_dout).cpu()
    assert torch.equal(dd[:, A:], torch.full((n, ld_dout - A), oc.SENT)), "padding columns of d_out written"
    _close(dd[:, :A], ref["d_out"], case["family"], "d_out")
    _word(loss[0], ref["loss"], oc.log_tol(ref["terms"]), "loss_out")
    if total is not None:
        _tail_ok(total, 1, "add_to")
        _word(total[0], ref["total"], oc.log_tol(ref["terms"] * case["coeff"]), "add_to")


@pytest.mark.parametrize("cid", oc.ids("actor_adv"))
def test_actor_loss_bwd_adv(ssa, cid):
    case, inp, ref = oc.load("actor_adv", cid)
    n, N = case["n"], case["nets"]
    q, logp, adv, la = (inp[k].to(DEV) for k in ("q", "logp", "adv", "log_alpha"))
    pop = _popart(ssa, case["popart"])
    dq, logs = _buf(N * n), _buf(1, [oc.PRE])
    ssa._lib.check(ssa._lib.lib.ssac_actor_loss_bwd_adv(
        q.data_ptr(), N, n, logp.data_ptr(), la.data_ptr(), case["ent"], pop.ptr if pop else 0, case["pop"], case["inv"],
        adv.data_ptr(), dq.data_ptr(), logs.data_ptr(), ssa.engine.stream()))
    _tail_ok(dq, N * n, "dq")
    _tail_ok(logs, 1, "logs")
    got = dq[:N * n].view(N, n).cpu()
    assert torch.equal(got != 0.0, ref["route"]), "dq is routed to the arg-min critic of every row and nowhere else"
    _close(got, ref["dq"], case["family"], "dq")
    _word(logs[0], ref["logs"], oc.log_tol(ref["terms"]), "logs[0] (from adv, not from Q)")


@pytest.mark.parametrize("cid", oc.ids("dr3"))
def test_dr3_add(ssa, cid):
    case, inp, ref = oc.load("dr3", cid)
    N, B, H = case["N"], case["B"], case["H"]
    blocks = ssa._lib.lib.ssac_dr3_blocks()
    assert blocks * 256 == oc.DR3_GRID   # (the shapes sit below, at and above one pass of this grid)
    h2, numel = inp["h2"].to(DEV), N * 2 * B * H
    dz2, partial = _buf(numel, inp["dz2"]), _buf(blocks, torch.full((blocks,), float("nan")))
    ssa._lib.check(ssa._lib.lib.ssac_dr3_add(dz2.data_ptr(), h2.data_ptr(), N, B, H, oc.DR3_COEF, partial.data_ptr(),
                                             ssa.engine.stream()))
    _tail_ok(dz2, numel, "dz2")
    _tail_ok(partial, blocks, "partial")
    got = dz2[:numel].cpu().view(N, 2 * B, H)
    _close(got, ref["dz2"], case["family"], "dz2")
    dead = inp["h2"] == 0.0   # behind a closed ReLU nothing is added: bit for bit what was there
    assert 0.4 < float(dead.float().mean()) < 0.6 and torch.equal(got[dead], inp["dz2"][dead])
    parts = partial[:blocks].cpu().double()
    assert bool(torch.isfinite(parts).all()), "every per-block partial is written"
    _word(parts.sum() / (N * B), ref["dot"], oc.log_tol(ref["terms"]), "dr3_dotproduct")


def _weight_checks(case, ref, w, logs):
    n, fam = case["n"], case["family"]
    _tail_ok(w, n, "w")
    _tail_ok(logs, 4, "logs")
    got, lg, rw = w[:n].cpu(), logs[:4].cpu(), ref["w"]
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(lg).all())
    _close(got, rw, fam, "w")
    elem = oc.atol_of(rw) + oc.rtol(fam) * float(rw.abs().max())
    _word(lg[0], ref["logs"][0], oc.log_tol(ref["terms"]), "mean")
    _word(lg[1], ref["logs"][1], elem, "max")
    _word(lg[2], ref["logs"][2], oc.atol_of(rw) + oc.rtol(fam) * float(rw.abs().min()), "min")
    _word(lg[3], ref["logs"][3], oc.std_tol(rw, fam), "std")
    if n == 1:
        assert float(lg[3]) == 0.0
    return got


@pytest.mark.parametrize("cid", oc.ids("softmax"))
def test_softmax_weights(ssa, cid):
    case, inp, ref = oc.load("softmax", cid)
    n = case["n"]
    q, w, logs = inp["q"].to(DEV), _buf(n), _buf(4)
    ssa._lib.check(ssa._lib.lib.ssac_softmax_weights(q.data_ptr(), case["E"], n, case["temp"], w.data_ptr(), logs.data_ptr(),
                                                     ssa.engine.stream()))
    got = _weight_checks(case, ref, w, logs)
    _word(got.double().sum() / n, 1.0, oc.log_tol(ref["terms"]), "sum(w) / n_rows")
    if case["temp"] == 2000.0 and n > 1:
        assert float((got == 0.0).float().mean()) > 0.5, "the case is meant to underflow most weights"
    if n == 1:
        assert float(got[0]) == 1.0


@pytest.mark.parametrize("cid", oc.ids("sunrise"))
def test_sunrise_weights_row_ladder(ssa, cid):
    case, inp, ref = oc.load("sunrise", cid)
    n = case["n"]
    q, w, logs = inp["q"].to(DEV), _buf(n), _buf(4)
    ssa._lib.check(ssa._lib.lib.ssac_sunrise_weights(q.data_ptr(), case["E"], n, case["temp"], w.data_ptr(), logs.data_ptr(),
                                                     ssa.engine.stream()))
    _weight_checks(case, ref, w, logs)


@pytest.mark.parametrize("cid", oc.ids("min_select"))
def test_ensemble_min_select(ssa, cid):
    case, inp, ref = oc.load("min_select", cid)
    n, qd = case["n"], case["qd"]
    n_out = n if case["act"] else n * qd
    q, act, out = inp["q"].to(DEV), _dev(inp["act"]), _buf(n_out)
    ssa._lib.check(ssa._lib.lib.ssac_ensemble_min_select(q.data_ptr(), case["nets"], n, qd, _ptr(act), case["ld"],
                                                         out.data_ptr(), ssa.engine.stream()))
    _tail_ok(out, n_out, "out")
    _exact(out[:n_out].view(ref["out"].shape), ref["out"], "min over the nets, then gather")
