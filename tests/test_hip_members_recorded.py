"""GPU: recorded critic updates of agents with ensemble_size > 1 (SUNRISE: learning_utils.members_recordable, DESIGN.md
7f) against the eager path, the per-member weight form, the oracle, and a checkpoint resume.

Every run does GRAPH_WARMUP + 6 critic updates with a Polyak step of every member behind every second one: the eager
warm-up calls, the recording call, five updates through the C step (ssac_step_run_aux: the slot's aux word carries the
member whose gradient norm is logged).  Hook mode injects indices, subsets and normals by call count (the E eps buffers of
the recording are refilled in member order); stock mode holds the recorded and the eager Philox stream against each other
(member i at draw number d0 + i).  All engine-against-engine comparisons are bit for bit, Python's and torch's CPU
generator included.  Shapes: the `sunrise` fixture's (obs 11, act 3, hidden 64, N 2, n 2, E 3, B 64, 1 000 rows), its
discrete sibling `sunrise_discrete` (gradient clipping at 40: the joint norm over all members), E = 2 without backup
weights, and sunrise.gin's own shape (E 5, hidden 256, B 256, obs 17, act 6) for the C step alone."""
import copy
import functools
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import case_runner
import synth

pytestmark = pytest.mark.gpu
orc = case_runner.orc
_SUN = dict(synth.CASES["sunrise"])
CASES = {
    "sunrise": dict(_SUN),
    "sunrise_discrete": dict(synth.CASES["sunrise_discrete"], clip=40.0),
    "two_members_unweighted": dict(_SUN, E=2, weight_type=None, temp=None, seed=41),
    "sunrise_gin": dict(_SUN, obs=17, act=6, hidden=256, E=5, B=256, rows=2000, cap=2048, seed=42),
}
SEED = 0x5EED5EED
N_EXTRA = 6   # updates behind the warm-up: the recording call + five replays


def _n_upd():
    import super_sac_amd as ssa
    return ssa.learning.GRAPH_WARMUP + N_EXTRA


class _CountedDraws:
    """rng hooks that serve indices, subsets and normals from seeded generators, by call count (the idea of
    tests/test_hip_explore_recorded.py); Python's random keeps the gradient-norm pick"""

    def __init__(self, ssa, device):
        self.rng, self.device, self.n = ssa.rng, device, {"idx": 0, "sub": 0, "normal": 0}
        self.saved = (ssa.rng.draw_indices, ssa.rng.draw_subset, ssa.rng.draw_normal, ssa.rng.draw_normal_into)

    def _count(self, what):
        self.n[what] += 1
        return self.n[what]

    def _normal(self, shape):
        g = torch.Generator().manual_seed(1000 + self._count("normal"))
        return torch.randn(*shape, generator=g)

    def install(self):
        r = self.rng
        r.draw_indices = lambda n, b: torch.randint(n, (b,), generator=torch.Generator().manual_seed(2000 + self._count("idx")))
        r.draw_subset = lambda n, k: random.Random(3000 + self._count("sub")).sample(range(n), k)
        r.draw_normal = lambda shape, device: self._normal(shape).to(self.device)
        r.draw_normal_into = lambda dst: dst.copy_(self._normal(tuple(dst.shape)))

    def restore(self):
        r = self.rng
        r.draw_indices, r.draw_subset, r.draw_normal, r.draw_normal_into = self.saved


def _seed(s):
    torch.manual_seed(s); np.random.seed(s); random.seed(s); torch.cuda.manual_seed(s)


def _setup(ssa, cfg, dev, variant=None, precision=None):
    """variant: None (the case's agent with the fixtures' seeded weights), "beta" (Agent(beta_dist=True)) or "mlp-encoder"
    (a trainable two-layer encoder in front of it) -- freshly initialised agents of the same shape"""
    _seed(cfg["seed"])
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    if variant is None:
        agent = case_runner.build_engine_agent(cfg, dev)
    else:
        enc = (ssa.nets.MlpEncoder(cfg["obs"], 32, cfg["obs"]) if variant == "mlp-encoder"
               else ssa.nets.IdentityEncoder(cfg["obs"]))
        agent = ssa.Agent(act_space_size=cfg["act"], encoder=enc, actor_network_cls=ssa.nets.ContinuousStochasticActor,
                          critic_network_cls=ssa.nets.ContinuousCritic, discrete=False, ensemble_size=cfg["E"],
                          num_critics=cfg["N"], ucb_bonus=0.0, hidden_size=cfg["hidden"], auto_rescale_targets=False,
                          log_std_low=cfg["lo"], log_std_high=cfg["hi"], beta_dist=variant == "beta")
        agent.to(dev)
        agent.train()
    if precision:
        ssa.set_precision(agent, precision)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    las = []
    for _ in range(agent.ensemble_size):
        la = torch.Tensor([math.log(cfg["init_alpha"])]).to(dev)
        la.requires_grad = True
        las.append(la)
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(cfg["B"])])
    agent.__dict__["_ssac_noise"] = [SEED, 0, 0]
    _seed(cfg["seed"] + 1)
    return buf, agent, target, copt, eopt, las, aug


def _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug, per=False, weight_type="cfg"):
    return ssa.learning.critic_update(
        buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
        batch_size=cfg["B"], gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
        target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=cfg["temp"],
        weight_type=cfg["weight_type"] if weight_type == "cfg" else weight_type, pop=bool(cfg.get("pop")),
        augmenter=aug, encoder_lambda=0, aug_mix=0.0, discrete=cfg["discrete"], random_process=None,
        noise_clip=None, per=per, update_priorities=False, dr3_coeff=0.0)


def _polyak(ssa, cfg, agent, target):
    for i in range(agent.ensemble_size):
        ssa.learning_utils.soft_update(target.critics[i], agent.critics[i], cfg["tau"])


def _weights(agent, cfg):
    """the backup weights the update just issued left in the agent's workspace: (E, B), whichever form wrote them"""
    bufs = agent.__dict__["_ssac_ws"]._bufs
    E, B = cfg["E"], cfg["B"]
    if ("bw.wall", (E, B), torch.float32) in bufs:
        return bufs[("bw.wall", (E, B), torch.float32)].clone()
    return torch.stack([bufs[(f"bw.w{i}", (B, 1), torch.float32)].view(B) for i in range(E)])


def _final(ssa, cfg, dev, out, agent, target, copt):
    for i in range(agent.ensemble_size):
        ar = agent.critics[i].arena(dev)
        m, v = copt._ssac_adam.moments_for(("critic", i), ar.params)
        out[f"adam_m{i}"], out[f"adam_v{i}"] = m.clone(), v.clone()
        out[f"critic{i}"] = torch.cat([p.detach().flatten() for p in agent.critics[i].parameters()])
        out[f"target{i}"] = torch.cat([p.detach().flatten() for p in target.critics[i].parameters()])
    torch.cuda.synchronize()
    out["py_random"] = np.frombuffer(repr(random.getstate()).encode(), np.uint8).copy()
    out["torch_rng"] = torch.get_rng_state().numpy().copy()
    return {k_: (v_.cpu().numpy() if torch.is_tensor(v_) else v_) for k_, v_ in out.items()}


@functools.lru_cache(maxsize=None)
def _run(case, hook, recorded, packed=True, toggle=False, resume=None):
    """hook: every index / subset / normal injected by call count.  toggle: the hook is removed behind update
    GRAPH_WARMUP + 1 and installed again behind GRAPH_WARMUP + 3 (started as `hook` says).  resume: a directory -- the run
    saves its training state behind update GRAPH_WARMUP + 2 and goes on in FRESH objects loaded from it.  Returns what the
    paths must agree on, as host arrays (computed once per argument tuple, never modified)."""
    import super_sac_amd as ssa
    L, lu = ssa.learning, ssa.learning_utils
    cfg, dev = CASES[case], torch.device("cuda")
    n_upd, W = _n_upd(), L.GRAPH_WARMUP
    old = (L.USE_GRAPHS, lu.PACKED_WEIGHTS)
    L.USE_GRAPHS, lu.PACKED_WEIGHTS = recorded, packed
    draws = _CountedDraws(ssa, dev)
    try:
        buf, agent, target, copt, eopt, las, aug = _setup(ssa, cfg, dev)
        hooked = False
        if hook:
            draws.install()
            hooked = True
        out, kept, picks, noise = {}, [], [], []
        for k in range(n_upd):
            logs, dicts = _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug)
            for i, rd in enumerate(dicts):
                out[f"td{k}_{i}"] = rd["td_target"].clone()
                out[f"idx{k}_{i}"] = np.array(rd["priority_idxs"])
            if cfg["weight_type"] is not None:
                out[f"w{k}"] = _weights(agent, cfg)
            noise.append(agent.__dict__["_ssac_noise"][1])
            graphs = agent.__dict__.get("_ssac_graphs") or {}
            if graphs and k >= W:
                picks.append(next(iter(graphs.values())).pick)
            if k % 2 == 1:
                _polyak(ssa, cfg, agent, target)
            if k % 4 == 2:   # (some log values are looked at straight away, most long afterwards)
                out[f"logs{k}"] = {k_: float(v) for k_, v in logs.items()}
            else:
                kept.append((k, logs))
            if toggle and k in (W + 1, W + 3):
                (draws.restore if hooked else draws.install)()
                hooked = not hooked
            if resume is not None and k == W + 2:
                for k2, lg in kept:
                    out[f"logs{k2}"] = {k_: float(v) for k_, v in lg.items()}
                kept = []
                ssa.checkpoint.save_training_state(resume, agent, target, {"critic": copt}, las)
                buf, agent, target, copt, eopt, las, aug = _setup(ssa, cfg, dev)   # FRESH objects ...
                ssa.checkpoint.load_training_state(resume, agent, target, {"critic": copt}, las)   # ... and generators
        for k, lg in kept:
            out[f"logs{k}"] = {k_: float(v) for k_, v in lg.items()}
        out = _final(ssa, cfg, dev, out, agent, target, copt)
        out["noise_draws"] = np.array(noise)
        out["picks"] = np.array(picks)
        graphs, fast = agent.__dict__.get("_ssac_graphs") or {}, agent.__dict__.get("_ssac_fast") or {}
        if recorded and resume is None:
            # (on the code before this feature _ssac_graphs stays empty for ensemble_size > 1: these fail there)
            assert len(graphs) == 1, "the ensemble update was not recorded"
            record, = graphs.values()
            assert record.path == "fast" and fast, "the recording never reached the C step"
            assert record.fast is not None and record.fast in fast.values()
            assert record.n_members == cfg["E"] and record.k == n_upd - W
            out["list_size"] = sum(ssa._lib.lib.ssac_launch_list_size(p_) for p_ in record.graph.parts)
        elif not recorded:
            assert not graphs and not fast, "the eager run recorded"
        return out
    finally:
        L.USE_GRAPHS, lu.PACKED_WEIGHTS = old
        draws.restore()


_SKIP = ("list_size", "picks")


def _assert_same(a, b, what, only=None):
    keys = [k_ for k_ in a if k_ not in _SKIP and (only is None or k_.startswith(only))]
    assert sorted(keys) == sorted(k_ for k_ in b if k_ not in _SKIP and (only is None or k_.startswith(only)))
    for k_ in keys:
        if k_.startswith("logs"):
            assert a[k_] == b[k_], (what, k_, a[k_], b[k_])
            assert all(np.isfinite(v) for v in a[k_].values()), (what, k_)
        else:
            assert a[k_].dtype == b[k_].dtype and a[k_].shape == b[k_].shape, (what, k_)
            assert np.array_equal(a[k_].view(np.uint8), b[k_].view(np.uint8)), (what, k_)


SMALL = ["sunrise", "sunrise_discrete", "two_members_unweighted"]


@pytest.mark.parametrize("hook", [True, False], ids=["injected", "stock"])
@pytest.mark.parametrize("case", SMALL)
def test_recorded_equals_eager(case, hook):
    """every log value of every update, every member's TD target, all critic parameters, both Adam moments, the targets
    and the two CPU generators; on the recorded run exactly one recording, on the C step"""
    import super_sac_amd as ssa
    eager = _run(case, hook, False)
    rec = _run(case, hook, True)
    _assert_same(rec, eager, case)
    cfg, W = CASES[case], ssa.learning.GRAPH_WARMUP
    assert not np.array_equal(eager[f"td{W}_0"], eager[f"td{W + 1}_0"])   # (the updates are not copies of each other)
    assert not np.array_equal(eager[f"td{W}_0"], eager[f"td{W}_1"])       # (nor the members)
    if cfg["weight_type"] is not None:
        assert "bellman_weights/mean" in eager[f"logs{W}"] and eager[f"w{W}"].std() > 0
    print(f"{case}: {rec['list_size']} library launches per recorded update")
    # the agent's noise stream: E draws per update, whoever issues it (stock: consumed in-kernel; hook: never touched)
    stochastic = cfg["actor"] == "stochastic"
    want = (np.arange(1, _n_upd() + 1) * cfg["E"]) if (stochastic and not hook) else np.zeros(_n_upd(), int)
    assert np.array_equal(rec["noise_draws"], want) and np.array_equal(eager["noise_draws"], want)


@pytest.mark.parametrize("case", SMALL)
def test_the_logged_gradient_norm_follows_the_pick(case):
    """gradients/critic_random_grad over the recorded updates equals the eager run's (which picks with random.choice and
    reads that member's norm), and the seed makes the recorded updates pick at least two different members: the recorded
    launches select the buffer on the device, by the slot's aux word"""
    import super_sac_amd as ssa
    W = ssa.learning.GRAPH_WARMUP
    for hook in (True, False):
        eager, rec = _run(case, hook, False), _run(case, hook, True)
        for k in range(W, _n_upd()):
            assert rec[f"logs{k}"]["gradients/critic_random_grad"] == eager[f"logs{k}"]["gradients/critic_random_grad"]
        assert len(rec["picks"]) == N_EXTRA and len(set(rec["picks"].tolist())) >= 2, rec["picks"]
        norms = [rec[f"logs{k}"]["gradients/critic_random_grad"] for k in range(W, _n_upd())]
        assert len(set(norms)) == len(norms) and all(v > 0 for v in norms)


@pytest.mark.parametrize("case", ["sunrise", "sunrise_discrete", "sunrise_gin"])
def test_packed_weights_off_gives_the_same_bits(case):
    """learning_utils.PACKED_WEIGHTS = False (E forwards + E ssac_ensemble_min_select + ssac_sunrise_weights per member
    batch, also recorded) against the packed form: the weights of every update, every log, the parameters afterwards.
    (sunrise_gin: the per-member forwards run on 16-row tiles there, the packed one on 32-row tiles.)"""
    packed, per_member = _run(case, False, True), _run(case, False, True, packed=False)
    _assert_same(per_member, packed, case)
    E = CASES[case]["E"]
    # E (2 E + 1) launches become the pack copy, the packed forward(s) and ssac_members_sunrise_weights
    forwards = {"sunrise": 1, "sunrise_discrete": 1, "sunrise_gin": 4}[case]   # (10 nets x 1 280 rows: groups of 3 nets)
    assert per_member["list_size"] - packed["list_size"] == E * (2 * E + 1) - (2 + forwards), \
        (per_member["list_size"], packed["list_size"])
    _assert_same(_run(case, False, False, packed=False), packed, case + " eager")


def test_a_hook_that_comes_and_goes_records_again():
    for start in (True, False):
        eager, rec = _run("sunrise", start, False, toggle=True), _run("sunrise", start, True, toggle=True)
        _assert_same(rec, eager, f"toggle from {start}")
    assert not np.array_equal(_run("sunrise", True, True, toggle=True)["critic0"], _run("sunrise", True, True)["critic0"])


def test_checkpoint_resume_equals_the_uninterrupted_run(tmp_path_factory):
    """save_training_state behind update GRAPH_WARMUP + 2 (two of them through the C step), fresh objects, load: the
    remaining updates equal the uninterrupted recorded run's, and the noise stream went on from E draws per update"""
    path = str(tmp_path_factory.mktemp("members_ckpt"))
    whole = _run("sunrise", False, True)
    resumed = _run("sunrise", False, True, resume=path)
    _assert_same(resumed, whole, "resume")
    assert np.array_equal(whole["noise_draws"], np.arange(1, _n_upd() + 1) * CASES["sunrise"]["E"])


def test_the_c_step_runs_at_the_gym_config_shape():
    """sunrise.gin's own shape (E 5, hidden 256, B 256): recorded, on the C step, finite, and equal to the eager run"""
    rec, eager = _run("sunrise_gin", False, True), _run("sunrise_gin", False, False)
    _assert_same(rec, eager, "sunrise_gin")
    print(f"sunrise_gin: {rec['list_size']} library launches per recorded update")


# ------------------------------------------------------------------------------------------ oracle parity
N_ORACLE = 3 + 3   # GRAPH_WARMUP (asserted) + the recording call and two replays
ORACLE_CASES = ["sunrise", "sunrise_discrete"]


@functools.lru_cache(maxsize=None)
def _oracle_draws(case):
    cfg = CASES[case]
    g = torch.Generator().manual_seed(cfg["seed"] + 500)
    py = random.Random(cfg["seed"] + 501)
    steps = []
    for _ in range(N_ORACLE):
        st = dict(idx=[torch.randint(cfg["rows"], (cfg["B"],), generator=g).numpy() for _ in range(cfg["E"])],
                  subset=[py.sample(range(cfg["N"]), cfg["n"]) for _ in range(cfg["E"])], pick=py.randrange(cfg["E"]))
        if not cfg["discrete"]:
            st["eps"] = [torch.randn(cfg["B"], cfg["act"], generator=g).numpy() for _ in range(cfg["E"])]
        steps.append(st)
    return steps


def _run_oracle(case):
    cfg, B, E = CASES[case], CASES[case]["B"], CASES[case]["E"]
    _seed_cpu(cfg["seed"])
    obuf = orc.ReplayOracle(cfg["cap"])
    obuf.load_experience(*case_runner._buffers(cfg))
    oa = case_runner._oracle_agent(cfg)
    oa.requires_grad_(True)
    ot = oa.clone()
    copt = orc.AdamOracle(oa.critic_params(), lr=cfg["lr"])
    eopt = orc.AdamOracle(oa.encoder_params(), lr=1e-4)
    las = [torch.tensor([math.log(cfg["init_alpha"])], requires_grad=True) for _ in range(E)]
    aug = orc.AugOracle("identity", B)
    rec = {}
    for k, st in enumerate(_oracle_draws(case)):
        logs, dicts = orc.critic_update(
            obuf, oa, ot, copt, eopt, las, B, cfg["gamma"], cfg["clip"], cfg["clip"], cfg["n"], cfg["temp"],
            cfg["weight_type"], cfg["pop"], aug, aug_mix=0.0, idx_list=list(st["idx"]),
            eps_list=None if cfg["discrete"] else [torch.from_numpy(e) for e in st["eps"]],
            subset_list=[list(s) for s in st["subset"]], grad_pick=st["pick"])
        for i in range(E):
            rec[f"u{k}_td{i}"] = dicts[i]["td_target"].numpy()
        for key, v in logs.items():
            rec[f"u{k}_log:{key}"] = np.float64(v)
        if k % 2 == 1:
            orc.soft_update(ot.critic_params(), oa.critic_params(), cfg["tau"])
    rec["final_critic"] = case_runner._flat(oa.critic_params())
    rec["final_target_critic"] = case_runner._flat(ot.critic_params())
    return rec


def _seed_cpu(s):
    torch.manual_seed(s); np.random.seed(s); random.seed(s)


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return _run_oracle(case)   # computed once, shared, never modified


def _run_engine_on_oracle_draws(case, recorded):
    import super_sac_amd as ssa
    L = ssa.learning
    assert L.GRAPH_WARMUP + 3 == N_ORACLE
    cfg, dev = CASES[case], torch.device("cuda")
    buf, agent, target, copt, eopt, las, aug = _setup(ssa, cfg, dev)
    player = case_runner.DrawPlayer(dev)
    player.install(ssa.rng)
    old = L.USE_GRAPHS
    L.USE_GRAPHS = recorded
    rec = {}
    try:
        for k, st in enumerate(_oracle_draws(case)):
            player.idx.extend(st["idx"])
            player.sub.extend(st["subset"])
            if not cfg["discrete"]:
                player.normal.extend(st["eps"])
            player.picks.append(st["pick"])
            logs, dicts = _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug)
            assert not player.normal and not player.idx and not player.sub and not player.picks, \
                "the engine consumed a different number of draws"
            for i in range(cfg["E"]):
                rec[f"u{k}_td{i}"] = dicts[i]["td_target"].cpu().numpy()
            for key, v in logs.items():
                rec[f"u{k}_log:{key}"] = np.float64(float(v))
            if k % 2 == 1:
                _polyak(ssa, cfg, agent, target)
        graphs = agent.__dict__.get("_ssac_graphs") or {}
        if recorded:
            record, = graphs.values()
            assert record.k == 3 and record.path == "fast" and record.fast.calls == 2
        else:
            assert not graphs
    finally:
        L.USE_GRAPHS = old
        player.restore()
    rec["final_critic"] = case_runner._flat([p for c in agent.critics for p in c.parameters()])
    rec["final_target_critic"] = case_runner._flat([p for c in target.critics for p in c.parameters()])
    return rec


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_two_oracle_runs_agree_with_themselves(case):
    """the oracle is a function of the draws alone (nothing leaks from a global generator into its numbers)"""
    a = _oracle(case)
    random.seed(12345); torch.manual_seed(999); np.random.seed(7)
    b = _run_oracle(case)
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert all(np.isfinite(np.asarray(v)).all() for v in a.values())


@pytest.mark.parametrize("path", ["recorded", "eager"])
@pytest.mark.parametrize("case", ORACLE_CASES)
def test_ensemble_updates_match_the_oracle(case, path):
    """the reference's numbers (oracle/ssac_oracle.py on handed-over draws) within case_runner.compare's tolerances: TD
    targets 2e-4, logs 5e-4, parameters 3e-5"""
    worst = case_runner.compare(_run_engine_on_oracle_draws(case, path == "recorded"), _oracle(case), who=f"{case}/{path}")
    print(f"{case}/{path}: worst deviations {worst}")


# ------------------------------------------------------------------------------------------ what stays eager
@pytest.mark.parametrize("setting", ["softmax", "mlp-encoder", "beta", "bf16", "per", "hipgraph-mode"])
def test_gated_out_calls_stay_eager_and_run(setting):
    """(an agent of MAX_MEMBERS + 1 members cannot be put through an update at all -- learning._critic_update_eager
    asserts ensemble_size <= MAX_MEMBERS -- so that clause is held by the predicate's truth table alone,
    tests/test_members_recording_cpu.py)"""
    import super_sac_amd as ssa
    L = ssa.learning
    dev = torch.device("cuda")
    cfg = dict(CASES["sunrise"])
    old = L.LAUNCH_MODE
    L.LAUNCH_MODE = "graph" if setting == "hipgraph-mode" else old
    try:
        args = _setup(ssa, cfg, dev, variant=setting if setting in ("beta", "mlp-encoder") else None,
                      precision="bf16" if setting == "bf16" else None)
        buf, agent = args[0], args[1]
        before = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).clone()
        for _ in range(L.GRAPH_WARMUP + 2):
            logs, dicts = _update(ssa, cfg, *args, per=setting == "per",
                                  weight_type="softmax" if setting == "softmax" else "cfg")
        after = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()])
        assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
        assert all(np.isfinite(float(v)) for v in logs.values())
        assert not agent.__dict__.get("_ssac_graphs") and not agent.__dict__.get("_ssac_fast")
    finally:
        L.LAUNCH_MODE = old
