"""CPU: the inputs and float64 references of offline_head_cases.py are fit for purpose before any kernel sees them -- the grid
inputs are exact in float32, no advantage sits near the filter's threshold, the deterministic-head inputs stay where the heads
are well conditioned, the references agree with the CPU oracle where it has the quantity, and the float32 deviation of every
formula stays under the constants the GPU tolerances are derived from."""
import numpy as np
import pytest
import torch

import offline_head_cases as oc
import ssac_oracle as orc


def _all_cases(kernel):
    cases, make, ref, keys = oc.KERNELS[kernel]
    for c in cases:
        yield c, make(c), ref, keys


def test_every_kernel_walks_the_row_ladder():
    for kernel, (cases, *_rest) in oc.KERNELS.items():
        if kernel == "dr3":
            continue
        rows = {c["n"] for c in cases}
        assert {1, 65, 1025, 2500} <= rows, kernel
        assert rows <= set(oc.LADDER) | {70000}, kernel
        assert len({c["id"] for c in cases}) == len(cases)
    sizes = [c["N"] * c["B"] * c["H"] for c in oc.DR3]
    assert sizes[0] < oc.DR3_GRID == sizes[1] < sizes[2] and sizes[2] % oc.DR3_GRID != 0
    assert any(c["n"] * c["qd"] > 1024 * 256 and not c["act"] for c in oc.MIN_SELECT)


@pytest.mark.parametrize("kernel", ["adv_filter", "adv_filter_discrete"])
def test_grid_inputs_are_exact_in_float32_and_carry_zero_advantages(kernel):
    seen = 0
    for case, inp, ref, _ in _all_cases(kernel):
        if not case["exact"]:
            continue
        seen += 1
        r64, r32 = ref(inp, case, oc.F64), ref(inp, case, oc.F32)
        assert torch.equal(r32["adv"].double(), r64["adv"]) and torch.equal(r32["mask"].double(), r64["mask"])
        rows = oc._planted(case["n"])
        assert float(r64["adv"][rows].abs().max()) == 0.0 and bool((r64["mask"][rows] == 1.0).all())
        assert torch.equal(r32["prio"][rows], torch.full((len(rows),), 1e-4))
        if case["n"] > 60:   # the filter both passes and rejects rows
            assert 0.2 < float(r64["mask"].mean()) < 0.8
    assert seen >= 1


@pytest.mark.parametrize("kernel", ["adv_filter", "adv_filter_discrete"])
def test_no_advantage_near_the_filter_threshold(kernel):
    for case, inp, ref, _ in _all_cases(kernel):
        if case["exact"]:
            continue
        adv = ref(inp, case, oc.F64)["adv"]
        assert float(adv.abs().min()) >= 1e-4, case["id"]
        if case["n"] > 60:
            assert 0.2 < float((adv >= 0).double().mean()) < 0.8


def test_deterministic_head_inputs_are_well_conditioned():
    for case, inp, _, _ in _all_cases("bc_det"):
        A = case["A"]
        out, a = inp["out"][:, :A].double(), inp["act"][:, :A].double()
        assert float(out.abs().max()) <= oc.DET_OUT_MAX and float(a.abs().max()) <= 1.0
        assert float((a - torch.tanh(out)).abs().min()) >= oc.DET_GAP, case["id"]
    for case, inp, _, _ in _all_cases("actinv_det"):
        A = case["A"]
        oo, oa = inp["out_o"][:, :A].double(), inp["out_a"][:, :A].double()
        assert max(float(oo.abs().max()), float(oa.abs().max())) <= oc.DET_OUT_MAX
        assert float((torch.tanh(oo) - torch.tanh(oa)).abs().min()) >= oc.DET_GAP, case["id"]


def test_edge_inputs_are_present():
    seen = set()
    for case, inp, _, _ in _all_cases("bc_logprob"):
        seen |= set(inp["act"][:, :case["A"]].reshape(-1).tolist()) & {float(np.float32(v)) for v in oc.ACT_EDGES}
        assert float(inp["act"][:, :case["A"]].abs().max()) <= 1.0
    assert len(seen) == len(oc.ACT_EDGES)
    for kernel in ("bc_logprob", "bc_discrete", "bc_det"):
        cases = oc.KERNELS[kernel][0]
        assert {c["mask"] for c in cases} == {"none", "rand", "zero"} and {c["inv"] for c in cases} == {1.0, 0.5, 10.0}
        assert {c["pad"] for c in cases} == {0, 1} and {c["member"] for c in cases} == {0, 1}
    for case, inp, _, _ in _all_cases("bc_discrete"):
        if case["scale"] == 20.0 and case["n"] > 60:   # saturated rows
            assert float((torch.softmax(inp["logits"].double(), -1).max(-1).values > 1 - 1e-6).double().mean()) > 0.1
    for case, inp, _, _ in _all_cases("dr3"):
        assert 0.4 < float((inp["h2"] == 0).float().mean()) < 0.6 and float(inp["dz2"].abs().min()) > 0.0
    for case, inp, ref, _ in _all_cases("actor_adv"):
        if case["n"] > 60:   # the advantage is NOT the critics' value: a log built from Q misses the log tolerance
            r = ref(inp, case)
            q = inp["q"].double().min(0).values
            if case["popart"] and case["pop"]:
                q = case["popart"][0] * q + case["popart"][1]
            assert abs(float((q - inp["adv"].double()).mean()) * case["inv"]) > 100 * oc.log_tol(r["terms"])
    for case, inp, ref, _ in _all_cases("softmax"):
        if case["temp"] == 2000.0 and case["n"] > 1:
            assert float((ref(inp, case)["w"].float() == 0).float().mean()) > 0.5


def _agent(discrete, E, popart, seed):
    ag = orc.AgentOracle(state_dim=5, act_dim=3, hidden=16, num_critics=2, ensemble_size=E, discrete=discrete,
                         log_std_low=-5.0, log_std_high=2.0, popart=popart, seed=seed)
    if popart:
        for p in ag.popart:
            p.w, p.b = torch.tensor([oc.POP_GENERAL[0]]), torch.tensor([oc.POP_GENERAL[1]])
    return ag


@pytest.mark.parametrize("popart", [False, True])
def test_advantage_references_agree_with_the_oracle(popart):
    g = torch.Generator().manual_seed(5)
    B = 200
    o = {"obs": torch.randn(B, 5, generator=g)}
    # continuous: the critics' outputs on [data | 4 sampled actions], as the engine stacks them
    ag = _agent(False, 1, popart, 3)
    a = torch.tanh(torch.randn(B, 3, generator=g))
    eps = [torch.randn(B, 3, generator=g) for _ in range(4)]
    for method in ("mean", "max"):
        want = orc.advantage(ag, o, a, 0, eps, method)[:, 0]
        out = orc.mlp3(ag.actors[0], o["obs"])[0]
        acts = [a] + [orc.tanh_normal_sample(out, ag.lo, ag.hi, e)[0] for e in eps]
        q = torch.stack([torch.cat([orc.critic_q(p, o["obs"], x)[:, 0] for x in acts]) for p in ag.critics[0]])
        case = dict(n=B, nets=2, samp=4, max=int(method == "max"), popart=oc.POP_GENERAL if popart else None)
        got = oc.adv_filter_ref(dict(q=q), case)
        sure = want.abs() > 1e-5
        assert float((got["adv"] - want.double()).abs().max()) < 1e-5 and int(sure.sum()) > B - 5
        assert torch.equal(got["mask"][sure], (want >= 0.0).double()[sure])
        assert torch.allclose(got["prio"], (torch.relu(want) + 1e-4).double(), atol=1e-5)
    # discrete: V from the mean probabilities of ALL actors
    ag = _agent(True, 2, popart, 4)
    idx = torch.randint(0, 3, (B,), generator=g)
    want = orc.advantage(ag, o, idx[:, None].float(), 1)[:, 0]
    logits = torch.stack([orc.mlp3(ac, o["obs"])[0] for ac in ag.actors])
    q = torch.stack([orc.critic_q(p, o["obs"]) for p in ag.critics[1]])
    case = dict(n=B, nets=2, actors=2, A=3, ld=1, popart=oc.POP_GENERAL if popart else None)
    got = oc.adv_filter_discrete_ref(dict(q=q, logits=logits, idx=idx), case)
    sure = want.abs() > 1e-5
    assert float((got["adv"] - want.double()).abs().max()) < 1e-5 and int(sure.sum()) > B - 5
    assert torch.equal(got["mask"][sure], (want >= 0.0).double()[sure])


def test_log_probability_references_agree_with_the_oracle():
    """the oracle's own float32 evaluation lies within float32 rounding of the float64 terms"""
    for case, inp, ref, _ in _all_cases("bc_logprob"):
        if case["mask"] != "none":
            continue
        A = case["A"]
        want = orc.tanh_normal_log_prob_data(inp["out"][:, :2 * A], case["lo"], oc.BC_HI, inp["act"][:, :A])[:, 0]
        got = ref(inp, case)["terms"]
        assert float((got - want.double()).abs().max()) <= 1e-5 * float(got.abs().max())
    for case, inp, ref, _ in _all_cases("bc_det"):
        if case["mask"] != "none":
            continue
        A = case["A"]
        want = orc.det_normal_log_prob(inp["out"][:, :A], inp["act"][:, :A])[:, 0]
        got = ref(inp, case)["terms"]
        assert float((got - want.double()).abs().max()) <= 1e-5 * float(got.abs().max())
    for case, inp, ref, _ in _all_cases("bc_discrete"):
        if case["mask"] != "none":
            continue
        want = torch.log_softmax(inp["logits"], -1).gather(-1, inp["idx"][:, None])[:, 0]   # offline_actor_update's line
        got = ref(inp, case)["terms"]
        assert float((got - want.double()).abs().max()) <= 1e-5 * float(got.abs().max())


@pytest.mark.parametrize("kind", ["softmax", "sunrise"])
def test_weight_references_agree_with_the_oracle(kind):
    g = torch.Generator().manual_seed(9)
    B, E, temp = 150, 3, 20.0
    ag = _agent(False, E, False, 6)
    o, o1 = {"obs": torch.randn(B, 5, generator=g)}, {"obs": torch.randn(B, 5, generator=g)}
    a = torch.tanh(torch.randn(B, 3, generator=g))
    eps = [torch.randn(B, 3, generator=g) for _ in range(E)]
    logs = {}
    want = orc.compute_backup_weights(logs, (o, a, None, o1, None), ag, ag, kind, temp, B, eps_list=eps)[:, 0]
    if kind == "sunrise":
        q = torch.stack([orc.ensemble_q(c, o["obs"], a)[:, 0] for c in ag.critics])
        got = oc.sunrise_weights_ref(dict(q=q), dict(n=B, temp=temp))
    else:
        q = torch.stack([orc.ensemble_q(c, o1["obs"], orc.tanh_normal_sample(orc.mlp3(ac, o1["obs"])[0], ag.lo, ag.hi, e)[0])[:, 0]
                         for ac, c, e in zip(ag.actors, ag.critics, eps)])
        got = oc.softmax_weights_ref(dict(q=q), dict(n=B, temp=temp))
    assert torch.allclose(got["w"], want.double(), rtol=1e-4, atol=1e-6)
    names = ("mean", "max", "min", "std")
    assert np.allclose(got["logs"].numpy(), [logs[f"bellman_weights/{k}"] for k in names], rtol=1e-4, atol=1e-6)


def test_float32_deviation_stays_under_the_recorded_constants(capsys):
    """F32_DEV (offline_head_cases.py's table) bounds what the same formula gives in torch float32 on the CPU; the GPU tests'
    rtol is max(1e-5, 4 x) that"""
    worst = {f: 0.0 for f in oc.F32_DEV}
    for kernel, (cases, make, ref, keys) in oc.KERNELS.items():
        for case in cases:
            inp = make(case)
            r64, r32 = ref(inp, case, oc.F64), ref(inp, case, oc.F32)
            for key in keys:
                assert r32[key].dtype == torch.float32 and r64[key].dtype == torch.float64
                worst[case["family"]] = max(worst[case["family"]], oc.rel_dev(r32[key], r64[key]))
    with capsys.disabled():
        print()
        for f, d in worst.items():
            print(f"  {f:22s} measured {d:8.1e}   F32_DEV {oc.F32_DEV[f]:8.1e}   rtol {oc.rtol(f):8.1e}")
    for f, d in worst.items():
        assert d <= oc.F32_DEV[f], f
        assert oc.rtol(f) >= 1e-5
    assert {c["family"] for cases, *_ in oc.KERNELS.values() for c in cases if "family" in c} == set(oc.F32_DEV)


def test_selection_reference_is_min_then_gather():
    for case, inp, ref, _ in _all_cases("min_select"):
        r = ref(inp, case)["out"]
        assert torch.equal(r.float().double(), r)   # float32 values: the comparison with the kernel is bit for bit
        if case["act"]:
            assert r.shape == (case["n"],) and inp["act"].shape == (case["n"], case["ld"])
            assert torch.equal(inp["act"][:, 0].long(), inp["idx"])
