"""GPU: acting with a two-layer MLP encoder (the reference's --shared_encoder and visgrid encoders as stand-ins, and
ssa.nets.MlpEncoder): Agent.forward / Agent.sample_action on numpy observations take the recorded plan (acting._PLANS) --
the encoder's forward recorded in front of the rule's launches through MlpEncoderEngine.forward_ptr, in each of its three
forms -- and equal the general path: head outputs within the project's ATOL_GENERAL = 2e-5, greedy discrete actions equal
on every row whose top-two gap exceeds 4 x that, Python's ``random`` stream consumed alike, shapes and dtypes alike.  The
plan's arithmetic is pinned to the fp64 oracle (the in-kernel Philox normals regenerated through ssac_philox_normal) under
mlp_encoder_cases.measured_bound taken over the whole chain encoder -> actor -> head.

Observation seeds: for every batch below the fp64 oracle alone (CPU) leaves at least one row with a clear top-two gap, and
the UCB batches at least n - 1 rows with a UCB gap above 1e-4 (the tests assert both on the oracle's own numbers)."""
import copy
import random

import numpy as np
import pytest
import torch

import mlp_encoder_cases as mc
import ssac_oracle as orc
from test_hip_acting_fast import _calls, _eps_of_call

pytestmark = pytest.mark.gpu

ATOL_GENERAL = 2e-5   # tests/test_hip_acting_fast.py::test_pixel_agents_take_the_one_call_path_and_equal_the_general_path
DEV = torch.device("cuda")
CONFIGS = dict(sac=mc.CONFIGS["sac"], ensemble=mc.CONFIGS["ensemble"], visgrid=mc.CONFIGS["visgrid"],
               discrete_e2=dict(mc.CONFIGS["visgrid"], E=2, seed=6))   # two members: the discrete UCB rule
FORM_SWITCHES = {"layers": (False, False), "fused": ("all", False), "rows": (True, "all")}   # (USE_FUSED, USE_ROWS)
CFG = pytest.mark.parametrize("name", list(CONFIGS))
OWN = pytest.mark.parametrize("own", [False, True], ids=["adopted", "ssa.nets.MlpEncoder"])
FORMS = pytest.mark.parametrize("form", list(FORM_SWITCHES))


@pytest.fixture
def launch_form(form):
    from super_sac_amd import mlp_encoder as me
    saved = me.USE_FUSED, me.USE_ROWS
    me.USE_FUSED, me.USE_ROWS = FORM_SWITCHES[form]
    yield form
    me.USE_FUSED, me.USE_ROWS = saved


def _agent(name, own, ucb=0.0):
    agent = mc.engine_agent(orc, CONFIGS[name], DEV, own)
    agent.__dict__["_ssac_noise"] = [4321, 0, 0]
    agent.ucb_bonus = ucb
    return agent


def _obs(name, n, seed, count):
    rs = np.random.RandomState(seed)
    shape = CONFIGS[name]["obs"]
    return [rs.standard_normal(shape if n == 1 else (n,) + shape).astype(np.float32) for _ in range(count)]


def _oracles(name):
    """(fp32, fp64) oracle agents of a configuration"""
    out = []
    for dt in (torch.float32, torch.float64):
        oa = mc.oracle_agent(orc, CONFIGS[name], dt)
        oa.obs_shape = CONFIGS[name]["obs"]
        out.append(oa)
    return out


def _rep(oa, obs, n):
    """the oracle's encoding of a numpy observation, in the oracle agent's dtype"""
    x = torch.from_numpy(np.asarray(obs, np.float32)).reshape((n,) + tuple(oa.obs_shape))
    return mc.patched_encode(orc)(oa.encoder, {"obs": x})


def _within(what, got, pair):
    """|got - fp64| under measured_bound of the (fp32, fp64) oracle pair"""
    bound = mc.measured_bound(*pair)
    err = float(np.abs(np.asarray(got, np.float64) - pair[1].numpy()).max())
    print(f"{what}: |plan - fp64| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _general(fn):
    """fn() with the recorded path switched off"""
    from super_sac_amd import acting
    acting.ENABLED = False
    try:
        return fn()
    finally:
        acting.ENABLED = True


def _plans(agent):
    from super_sac_amd import acting
    return acting._PLANS.get(agent) or {}


def _took_the_form(agent, form):
    eng = agent.encoder.__dict__["_ssac_mlp"]
    rows = any(k[0] == "t.rows" for k in eng.ws._bufs)
    assert rows == (form == "rows"), f"form {form}: few-row scratch {'present' if rows else 'absent'}"


@pytest.mark.parametrize("n", [1, 4])
@CFG
@OWN
@FORMS
def test_forward_and_sample_action_take_the_plan_and_equal_the_general_path(launch_form, own, name, n):
    cfg = CONFIGS[name]
    agent = _agent(name, own)
    for obs in _obs(name, n, 40 + n, 3):   # (the first call records, the others replay)
        random.seed(5)
        fast = agent.forward({"obs": obs}, num_envs=n)
        fast_act, fast_dist = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        fast_state = random.getstate()
        plans = _plans(agent)
        assert ("forward", n, 0.0) in plans and ("sample", n, 0.0) in plans, "the calls did not take the recorded path"
        assert plans[("forward", n, 0.0)].mlp_in == int(np.prod(cfg["obs"])) and plans[("forward", n, 0.0)].pixel_shape is None
        random.seed(5)
        want = _general(lambda: agent.forward({"obs": obs}, num_envs=n))
        want_act, want_dist = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, return_dist=True))
        assert random.getstate() == fast_state, "the recorded path consumed Python's random stream differently"
        for got, ref in ((fast, want), (fast_act, want_act)):
            assert isinstance(got, np.ndarray) and got.shape == ref.shape and got.dtype == ref.dtype
        assert fast.shape == ((1,) if cfg["discrete"] else (cfg["act"],)) if n == 1 else fast.shape[0] == n
        assert fast_dist.shape == want_dist.shape and fast_dist.dtype == want_dist.dtype
        got, ref = fast_dist.detach().cpu().numpy().reshape(n, -1), want_dist.detach().cpu().numpy().reshape(n, -1)
        print(f"{name} n={n} head output: max deviation {np.abs(got - ref).max():.3e}")
        np.testing.assert_allclose(got, ref, atol=ATOL_GENERAL, rtol=0)
        if cfg["discrete"]:
            if cfg["E"] == 1:   # (one member: the greedy rule's mean probabilities are ordered as its logits)
                top = np.sort(ref, axis=1)
                clear = (top[:, -1] - top[:, -2]) > 4 * ATOL_GENERAL
                assert clear.any()
                assert np.array_equal(fast.reshape(n, -1)[clear], want.reshape(n, -1)[clear])
            assert 0 <= fast_act.min() and fast_act.max() < cfg["act"]
        else:
            np.testing.assert_allclose(fast.reshape(n, -1), want.reshape(n, -1), atol=ATOL_GENERAL, rtol=0)
            assert np.abs(fast_act).max() <= 1.0
    _took_the_form(agent, launch_form)


@pytest.mark.parametrize("n", [1, 4])
@OWN
@FORMS
def test_the_greedy_rule_of_a_discrete_ensemble_equals_the_general_path(launch_form, own, n):
    """two members: the arg-max of the MEAN probabilities, on rows where that mean has a clear top-two gap"""
    agent = _agent("discrete_e2", own)
    _, oa = _oracles("discrete_e2")
    for obs in _obs("discrete_e2", n, 60 + n, 3):
        fast = agent.forward({"obs": obs}, num_envs=n)
        assert ("forward", n, 0.0) in _plans(agent)
        want = _general(lambda: agent.forward({"obs": obs}, num_envs=n))
        rep = _rep(oa, obs, n)
        probs = torch.stack([torch.softmax(orc.mlp3(a, rep)[0], -1) for a in oa.actors], 0).mean(0)
        top = torch.sort(probs, dim=1).values
        clear = ((top[:, -1] - top[:, -2]) > 4 * ATOL_GENERAL).numpy()
        assert clear.any()
        assert np.array_equal(fast.reshape(n)[clear], want.reshape(n)[clear])
        assert np.array_equal(fast.reshape(n)[clear], probs.argmax(1).numpy()[clear])


@pytest.mark.parametrize("name", ["sac", "ensemble"])
@OWN
@FORMS
def test_continuous_plans_compute_the_reference_arithmetic(launch_form, own, name):
    cfg = CONFIGS[name]
    n, A, E = 4, cfg["act"], cfg["E"]
    agent = _agent(name, own)
    oa32, oa64 = _oracles(name)
    for rep_no, obs in enumerate(_obs(name, n, 77, 3)):
        # greedy: the mean over the members of tanh(mu)
        act = agent.forward({"obs": obs}, num_envs=n)
        refs = [torch.stack([torch.tanh(orc.mlp3(a, _rep(oa, obs, n))[0][:, :A]) for a in oa.actors], 0).mean(0)
                for oa in (oa32, oa64)]
        _within(f"{name} greedy", act, refs)
        # sample: the chosen member's tanh-normal draw on the plan's own Philox normals
        random.seed(100 + rep_no)
        k = random.choice(range(E))   # (the draw agent.sample_action is about to make: random.choice(self.actors))
        random.seed(100 + rep_no)
        act, dist = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        plan = _plans(agent)[("sample", n, 0.0)]
        eps = _eps_of_call(agent, plan, k, _calls(plan) - 1, n, A)
        outs = [orc.mlp3(oa.actors[k], _rep(oa, obs, n))[0] for oa in (oa32, oa64)]
        acts = [orc.tanh_normal_sample(o, oa32.lo, oa32.hi, eps.to(o.dtype))[0].clamp(-1, 1) for o in outs]
        _within(f"{name} sample", act, acts)
        _within(f"{name} head output", dist.cpu().numpy(), outs)


@OWN
@FORMS
def test_discrete_plans_compute_the_reference_arithmetic(launch_form, own):
    n = 4
    agent = _agent("visgrid", own)
    oa32, oa64 = _oracles("visgrid")
    for obs in _obs("visgrid", n, 78, 3):
        act = agent.forward({"obs": obs}, num_envs=n)
        _, logits = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        pair = [orc.mlp3(oa.actors[0], _rep(oa, obs, n))[0] for oa in (oa32, oa64)]
        _within("visgrid logits", logits.cpu().numpy(), pair)
        top = torch.sort(pair[1], dim=1).values
        clear = ((top[:, -1] - top[:, -2]) > 1e-4).numpy()
        assert clear.any()
        assert np.array_equal(act.reshape(n)[clear], pair[1].argmax(1).numpy()[clear])


@OWN
@FORMS
def test_ucb_picks_the_argmax_candidate_and_equals_the_general_path(launch_form, own):
    import super_sac_amd as ssa
    cfg = CONFIGS["ensemble"]
    n, E, A = 6, cfg["E"], cfg["act"]
    agent = _agent("ensemble", own, ucb=0.7)
    oas = _oracles("ensemble")
    oa = oas[1]
    for obs in _obs("ensemble", n, 3, 3):
        act = agent.sample_action({"obs": obs}, num_envs=n)
        plan = _plans(agent)[("ucb", n, 0.7)]
        call_no = _calls(plan) - 1
        eps = [_eps_of_call(agent, plan, a, call_no, n, A) for a in range(E)]
        s = _rep(oa, obs, n)
        cands32, cands = [torch.stack([orc.tanh_normal_sample(orc.mlp3(o.actors[a], _rep(o, obs, n))[0], o.lo, o.hi,
                                                              eps[a].to(o.actors[a]["w1"].dtype))[0] for a in range(E)], 0)
                          for o in oas]
        q = torch.stack([torch.stack([orc.ensemble_q(oa.critics[c], s, cands[a]).squeeze(-1) for a in range(E)], 0)
                         for c in range(E)], 0)                         # (members, candidates, envs)
        ucb = q.mean(0) + 0.7 * q.std(0)
        want = cands[ucb.argmax(0), torch.arange(n)].clamp(-1, 1)
        top2 = ucb.topk(2, dim=0).values
        clear = ((top2[0] - top2[1]) > 1e-4).numpy()   # (a near-tie may flip under fp32 reordering)
        assert clear.sum() >= n - 1
        bound = mc.measured_bound(cands32, cands)   # (the chosen candidate is one of these: the whole chain's distance)
        print(f"ucb: |plan - fp64| {np.abs(act[clear] - want.numpy()[clear]).max():.3e}, bound {bound:.3e}")
        np.testing.assert_allclose(act[clear], want.numpy()[clear], atol=bound, rtol=0)
        # the general path of agent.py on the same noise (the hook switches the recorded path off)
        queue = [e.clone() for e in eps]
        saved = ssa.rng.draw_normal
        ssa.rng.draw_normal = lambda shape, device: queue.pop(0).to(device)
        try:
            general = agent.sample_action({"obs": obs}, num_envs=n)
        finally:
            ssa.rng.draw_normal = saved
        assert not queue and _calls(plan) == call_no + 1, "the hooked call must have taken the general path"
        np.testing.assert_allclose(act[clear], general[clear], atol=ATOL_GENERAL, rtol=0)


@OWN
@FORMS
def test_the_discrete_ucb_rule_takes_the_plan(launch_form, own):
    cfg = CONFIGS["discrete_e2"]
    n = 6
    agent = _agent("discrete_e2", own, ucb=0.7)
    for obs in _obs("discrete_e2", n, 9, 3):
        random.seed(11)
        act, dist = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        state = random.getstate()
        assert ("sample", n, 0.7) in _plans(agent) and _plans(agent)[("sample", n, 0.7)].rule == "ducb"
        random.seed(11)
        want, want_dist = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, return_dist=True))
        assert random.getstate() == state
        assert act.shape == want.shape == (n, 1) and act.dtype == want.dtype and 0 <= act.min() and act.max() < cfg["act"]
        np.testing.assert_allclose(dist.cpu().numpy(), want_dist.cpu().numpy(), atol=ATOL_GENERAL, rtol=0)


@OWN
def test_the_plan_reads_the_weights_of_the_moment(own, tmp_path):
    from super_sac_amd import acting
    n, A = 4, CONFIGS["sac"]["act"]
    agent = _agent("sac", own)
    oas = _oracles("sac")
    obs = _obs("sac", n, 21, 1)[0]
    greedy = lambda: [torch.tanh(orc.mlp3(oa.actors[0], _rep(oa, obs, n))[0][:, :A]) for oa in oas]
    first = agent.forward({"obs": obs}, num_envs=n)
    plan = _plans(agent)[("forward", n, 0.0)]
    _within("greedy", first, greedy())
    # an in-place step on the encoder: the launches point into the arena
    with torch.no_grad():
        mc.encoder_tensors(agent.encoder)["b1"].add_(0.25)
    for oa in oas:
        oa.encoder["p"]["b1"] = oa.encoder["p"]["b1"] + 0.25
    moved = agent.forward({"obs": obs}, num_envs=n)
    assert _plans(agent)[("forward", n, 0.0)] is plan and _calls(plan) == 3   # (the recording pass, and two calls)
    assert np.abs(moved - first).max() > 1e-3
    _within("greedy after the step", moved, greedy())
    # save / load round trip: load_state_dict writes in place
    agent.save(str(tmp_path))
    with torch.no_grad():
        mc.encoder_tensors(agent.encoder)["b1"].add_(1.0)
    assert np.abs(agent.forward({"obs": obs}, num_envs=n) - moved).max() > 1e-3
    agent.load(str(tmp_path))
    assert np.array_equal(agent.forward({"obs": obs}, num_envs=n), moved)
    assert ("forward", n, 0.0) in _plans(agent)
    # a deep copy moves the weights: the plan is dropped and a new one recorded
    old = _plans(agent)[("forward", n, 0.0)]
    agent.encoder = copy.deepcopy(agent.encoder)
    again = agent.forward({"obs": obs}, num_envs=n)
    new = acting._PLANS[agent][("forward", n, 0.0)]
    assert new is not old and new.sig != old.sig
    assert np.array_equal(again, moved)


@OWN
def test_float64_and_grid_shaped_observations_take_the_same_plan_bit_for_bit(own):
    n = 4
    agent = _agent("visgrid", own)
    obs = _obs("visgrid", n, 31, 1)[0]
    assert obs.shape == (n, 18, 18)
    flat = obs.reshape(n, -1)
    a0 = agent.forward({"obs": flat}, num_envs=n)
    _, d0 = agent.sample_action({"obs": flat}, num_envs=n, return_dist=True)
    for other in (obs, obs.astype(np.float64), flat.astype(np.float64), np.asfortranarray(obs)):
        a = agent.forward({"obs": other}, num_envs=n)
        _, d = agent.sample_action({"obs": other}, num_envs=n, return_dist=True)
        assert np.array_equal(a, a0) and torch.equal(d, d0)
    assert set(_plans(agent)) == {("forward", n, 0.0), ("sample", n, 0.0)}
    assert _calls(_plans(agent)[("forward", n, 0.0)]) == 6   # (the recording pass and five calls: none left the plan)
    one = agent.forward({"obs": obs[0]}, num_envs=1)          # (18, 18) for one environment
    assert one.shape == (1,) and one[0] == a0[0, 0] and ("forward", 1, 0.0) in _plans(agent)


def test_rolling_shares_the_plan_of_a_pass_through_encoder_and_leaves_a_stateful_one_alone():
    import super_sac_amd as ssa
    n = 4
    agent = _agent("sac", True)
    obs = _obs("sac", n, 33, 1)[0]
    a0 = agent.forward({"obs": obs}, num_envs=n, rolling=False)
    a1 = agent.forward({"obs": obs}, num_envs=n, rolling=True)
    plan = _plans(agent)[("forward", n, 0.0)]
    assert np.array_equal(a0, a1) and len(_plans(agent)) == 1 and _calls(plan) == 3

    class Stateful(ssa.nets.MlpEncoder):
        def forward_rolling(self, obs):
            return self.forward(obs)
    cfg = CONFIGS["sac"]
    enc = Stateful(cfg["obs"], cfg["enc_hidden"], cfg["emb"], out_act=cfg["enc_act"])
    enc.load_state_dict(agent.encoder.state_dict())
    other = _agent("sac", True)
    other.encoder = enc.to(DEV)
    a2 = other.forward({"obs": obs}, num_envs=n, rolling=True)
    other.sample_action({"obs": obs}, num_envs=n, rolling=True)
    assert not _plans(other), "an encoder that overrides forward_rolling must act on the general path"
    np.testing.assert_allclose(a2, a0, atol=ATOL_GENERAL, rtol=0)
    # rolling=False is the stateless call of the same encoder: recorded
    other.forward({"obs": obs}, num_envs=n, rolling=False)
    assert ("forward", n, 0.0) in _plans(other)


@OWN
def test_what_stays_on_the_general_path_does_not_raise(own):
    import super_sac_amd as ssa
    n = 4
    agent = _agent("sac", own)
    obs = _obs("sac", n, 35, 1)[0]
    # injected noise: the hook draws it, the sample rule is not recorded
    saved = ssa.rng.draw_normal
    ssa.rng.draw_normal = lambda shape, device: torch.zeros(shape, device=device)
    try:
        act = agent.sample_action({"obs": obs}, num_envs=n)
    finally:
        ssa.rng.draw_normal = saved
    assert act.shape == (n, CONFIGS["sac"]["act"]) and ("sample", n, 0.0) not in _plans(agent)
    # from_cpu=False: tensors in, a tensor out
    t = agent.forward({"obs": torch.from_numpy(obs).to(DEV)}, from_cpu=False, num_envs=n)
    assert torch.is_tensor(t) and t.shape == (n, CONFIGS["sac"]["act"]) and not _plans(agent)
    # a bf16-marked network: what the update functions refuse for this encoder acts on the general path
    agent.actors[0].__dict__["_ssac_precision"] = "bf16"
    try:
        from super_sac_amd import acting
        assert not acting._eligible(agent, {"obs": obs}, n, False, False)
    finally:
        del agent.actors[0].__dict__["_ssac_precision"]
    greedy = agent.forward({"obs": obs}, num_envs=n)
    assert ("forward", n, 0.0) in _plans(agent)
    np.testing.assert_allclose(greedy, t.cpu().numpy(), atol=ATOL_GENERAL, rtol=0)


def test_a_failed_recording_hands_the_call_to_the_general_path(monkeypatch):
    from super_sac_amd import acting
    n = 4
    agent = _agent("ensemble", True)
    obs = _obs("ensemble", n, 37, 1)[0]
    random.seed(3)
    want = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, return_dist=True))
    state = random.getstate()

    def refuse(plan, agent_, which):
        raise RuntimeError("libssac_hip: refused for the test")
    monkeypatch.setattr(acting, "_record_launches", refuse)
    random.seed(3)
    with pytest.warns(RuntimeWarning, match="take the general path"):
        got = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
    assert random.getstate() == state, "the host draw of the failed recording was not handed back"
    assert ("sample", n, 0.0) in acting._FAILED[agent] and not _plans(agent)
    assert got[0].shape == want[0].shape and torch.equal(got[1], want[1])


@OWN
def test_acting_between_two_updates_disturbs_nothing_the_updates_keep(own):
    from super_sac_amd import encoder_base

    def two_updates(act_between):
        run = mc.EngineRun(orc, CONFIGS["sac"], "sac", device=DEV, own=own)
        run.agent.__dict__["_ssac_noise"] = [4321, 0, 0]
        obs = _obs("sac", 4, 39, 1)[0]
        for k in (0, 1):
            run.player.install(run.ssa.rng)
            try:
                run._critic(k, run.draws[k])
            finally:
                run.player.restore()
            if k == 0 and act_between:
                eng = encoder_base.encoder_engine(run.agent.encoder, DEV)
                kept = {} if eng.saved is None else {k: v.clone() for k, v in eng.saved.items() if torch.is_tensor(v)}
                state = random.getstate()
                run.agent.forward({"obs": obs}, num_envs=4)
                run.agent.sample_action({"obs": obs}, num_envs=4)
                random.setstate(state)
                assert len(_plans(run.agent)) == 2
                for k, v in kept.items():
                    assert torch.equal(eng.saved[k], v), f"the acting calls wrote into saved[{k!r}]"
        return run.finish()
    plain, acted = two_updates(False), two_updates(True)
    assert set(plain) == set(acted)
    for key in plain:
        assert np.array_equal(np.asarray(plain[key]), np.asarray(acted[key])), f"{key} differs after the acting calls"
