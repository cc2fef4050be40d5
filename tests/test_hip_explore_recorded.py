"""GPU: recorded critic updates that carry an exploration process (TD3 / DDPG / AWAC shapes) against the eager path.

Every run does 12 critic updates with a Polyak step behind every second one: three eager warm-up calls, the recording
call, eight updates through the C step (ssac_step_run_aux).  The process's scale is changed before EVERY update -- the
recorded launch reads it from the slot's aux word, so a recording that baked the scale in fails here -- and noise_clip
is set.  Hook mode (indices, subsets and normals injected by call count) holds the recorded launch
(ssac_explore_action) against the eager two-kernel sequence; the stock mode holds the recorded and the eager Philox
stream against each other.  All comparisons are bit for bit."""
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
N_UPD = 12
SEED = 0x5EED5EED
CASES = {
    "td3": dict(synth.CASES["td3_noise"]),                                 # deterministic head, N 2, n 2
    "sac_process": dict(synth.CASES["sac_noise"]),                         # tanh-normal head + process (AWAC)
    "ddpg": dict(synth.CASES["td3_noise"], N=1, n=1, seed=115),            # one critic
}
# the scale of update k: annealed, with jumps, never constant over two updates
SCHEDULES = {
    "anneal": [0.7 - 0.05 * k + (0.2 if k % 3 == 0 else 0.0) for k in range(N_UPD)],
    # the same up to and including the recording call (update 3), then another schedule
    "late-change": [0.7 - 0.05 * k + (0.2 if k % 3 == 0 else 0.0) + (0.25 if k >= 5 else 0.0) for k in range(N_UPD)],
}


class _CountedDraws:
    """rng hooks that serve indices, subsets and normals from seeded generators, by call count"""

    def __init__(self, ssa, device):
        self.rng, self.device, self.n = ssa.rng, device, {"idx": 0, "sub": 0, "normal": 0}
        self.saved = (ssa.rng.draw_indices, ssa.rng.draw_subset, ssa.rng.draw_normal, ssa.rng.draw_normal_into)

    def _count(self, what):
        self.n[what] += 1
        return self.n[what]

    def _normal(self, shape):
        g = torch.Generator().manual_seed(1000 + self._count("normal"))
        return torch.randn(*shape, generator=g)

    def install(self, normals_only=False):
        r = self.rng
        if not normals_only:
            r.draw_indices = lambda n, b: torch.randint(n, (b,), generator=torch.Generator().manual_seed(2000 + self._count("idx")))
            r.draw_subset = lambda n, k: random.Random(3000 + self._count("sub")).sample(range(n), k)
        r.draw_normal = lambda shape, device: self._normal(shape).to(self.device)
        r.draw_normal_into = lambda dst: dst.copy_(self._normal(tuple(dst.shape)))

    def remove_normals(self):
        self.rng.draw_normal, self.rng.draw_normal_into = self.saved[2:]

    def restore(self):
        r = self.rng
        r.draw_indices, r.draw_subset, r.draw_normal, r.draw_normal_into = self.saved


def _setup(ssa, cfg, dev, beta=False):
    torch.manual_seed(cfg["seed"]); np.random.seed(cfg["seed"]); random.seed(cfg["seed"]); torch.cuda.manual_seed(cfg["seed"])
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    if beta:
        agent = ssa.Agent(act_space_size=cfg["act"], encoder=ssa.nets.IdentityEncoder(cfg["obs"]),
                          actor_network_cls=ssa.nets.ContinuousStochasticActor,
                          critic_network_cls=ssa.nets.ContinuousCritic, ensemble_size=1, num_critics=cfg["N"],
                          hidden_size=cfg["hidden"], auto_rescale_targets=False, beta_dist=True)
        agent.to(dev)
    else:
        agent = case_runner.build_engine_agent(cfg, dev)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    las = []
    for _ in range(agent.ensemble_size):
        la = torch.Tensor([math.log(max(cfg["init_alpha"], 1e-15))]).to(dev)
        la.requires_grad = True
        las.append(la)
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(cfg["B"])])
    space = type("Space", (), {})()
    space.low, space.high = -np.ones(cfg["act"], np.float32), np.ones(cfg["act"], np.float32)
    rp = ssa.learning_utils.GaussianExplorationNoise(space, start_scale=1.0, final_scale=0.1, steps_annealed=1000)
    agent.__dict__["_ssac_noise"] = [SEED, 0, 0]
    torch.manual_seed(cfg["seed"] + 1); np.random.seed(cfg["seed"] + 1); random.seed(cfg["seed"] + 1)
    torch.cuda.manual_seed(cfg["seed"] + 1)
    return buf, agent, target, copt, eopt, las, aug, rp


def _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug, rp, per=False):
    return ssa.learning.critic_update(
        buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
        batch_size=cfg["B"], gamma=cfg["gamma"], critic_clip=None, encoder_clip=None, target_critic_ensemble_n=cfg["n"],
        weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
        discrete=False, random_process=rp, noise_clip=cfg["noise"]["clip"], per=per, update_priorities=False,
        dr3_coeff=0.0)


@functools.lru_cache(maxsize=None)
def _run(case, hook, recorded, schedule, hook_window=None, n_upd=N_UPD):
    """hook: every draw injected by call count for the whole run.  hook_window=(on, off): a stock run whose NORMALS are
    injected for the calls on <= k < off.  Returns what the two paths must agree on, as host arrays."""
    import super_sac_amd as ssa
    L = ssa.learning
    cfg, dev = CASES[case], torch.device("cuda")
    scales = SCHEDULES[schedule]
    old = L.USE_GRAPHS
    L.USE_GRAPHS = recorded
    draws = _CountedDraws(ssa, dev)
    try:
        buf, agent, target, copt, eopt, las, aug, rp = _setup(ssa, cfg, dev)
        if hook:
            draws.install()
        out, kept, steps = {}, [], []
        for k in range(n_upd):
            if hook_window and k == hook_window[0]:
                draws.install(normals_only=True)
            if hook_window and k == hook_window[1]:
                draws.remove_normals()
            rp.current_scale = scales[k % len(scales)]
            logs, dicts = _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug, rp)
            out[f"td{k}"] = dicts[0]["td_target"].clone()
            out[f"idx{k}"] = np.array(dicts[0]["priority_idxs"])
            if k % 2 == 1:
                ssa.learning_utils.soft_update(target.critics[0], agent.critics[0], cfg["tau"])
            if k % 5 == 3:   # (some log values are looked at straight away, most long afterwards)
                out[f"logs{k}"] = {k_: float(v) for k_, v in logs.items()}
            else:
                kept.append((k, logs))
            if recorded and hook_window and k in (hook_window[0] - 1, hook_window[0], hook_window[1] - 1, hook_window[1],
                                                  n_upd - 1):
                record, = agent.__dict__["_ssac_graphs"].values()
                steps.append((record.fast, record.in_kernel_noise, record.k))
        for k, lg in kept:
            out[f"logs{k}"] = {k_: float(v) for k_, v in lg.items()}
        ar = agent.critics[0].arena(dev)
        m, v = copt._ssac_adam.moments_for(("critic", 0), ar.params)
        out["adam_m"], out["adam_v"] = m.clone(), v.clone()
        out["critic"] = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()])
        out["target"] = torch.cat([p.detach().flatten() for p in target.critics[0].parameters()])
        torch.cuda.synchronize()
        out = {k_: (v_.cpu().numpy() if torch.is_tensor(v_) else v_) for k_, v_ in out.items()}
        if recorded:
            record, = agent.__dict__["_ssac_graphs"].values()
            step, = agent.__dict__["_ssac_fast"].values()
            assert step is record.fast and record.path == "fast" and record.k == n_upd - L.GRAPH_WARMUP
            assert record.proc_dev is not None and record.refs[4] is rp
            if not hook_window:
                assert step.calls == n_upd - L.GRAPH_WARMUP - 1
                assert record.in_kernel_noise == (not hook)
            out["steps"] = steps
            out["list_size"] = sum(ssa._lib.lib.ssac_launch_list_size(p_) for p_ in record.graph.parts)
        else:
            assert not agent.__dict__.get("_ssac_graphs") and not agent.__dict__.get("_ssac_fast"), "the eager run recorded"
        return out
    finally:
        L.USE_GRAPHS = old
        draws.restore()


def _assert_same(a, b, what):
    keys = [k_ for k_ in a if k_ not in ("steps", "list_size")]
    assert sorted(keys) == sorted(k_ for k_ in b if k_ not in ("steps", "list_size"))
    for k_ in keys:
        if k_.startswith("logs"):
            assert a[k_] == b[k_], (what, k_, a[k_], b[k_])
            assert all(np.isfinite(v) for v in a[k_].values()), (what, k_)
        else:
            assert a[k_].dtype == b[k_].dtype and np.array_equal(a[k_].view(np.uint8), b[k_].view(np.uint8)), (what, k_)


@pytest.mark.parametrize("case", sorted(CASES))
def test_recorded_equals_eager_under_injected_draws(case):
    """the recorded ssac_explore_action launch (fixed-address noise buffers, scale from the slot) against the eager
    ssac_tanh_normal_fwd + ssac_exploration_noise / ssac_det_action_fwd sequence (by-value scale)"""
    eager = _run(case, True, False, "anneal")
    rec = _run(case, True, True, "anneal")
    _assert_same(rec, eager, case)
    assert not np.array_equal(eager["td3"], eager["td4"])   # (the updates are not copies of each other)


@pytest.mark.parametrize("case", sorted(CASES))
def test_recorded_equals_eager_on_the_stock_philox_stream(case):
    """no hook: warm-up calls (host draw number) and recorded calls (draw number from the slot) follow one stream"""
    eager = _run(case, False, False, "anneal")
    rec = _run(case, False, True, "anneal")
    _assert_same(rec, eager, case)
    hooked = _run(case, True, False, "anneal")
    assert not np.array_equal(eager["td0"], hooked["td0"])   # (another noise source, other numbers)


@pytest.mark.parametrize("case", ["td3", "sac_process"])
def test_a_scale_changed_after_the_recording_reaches_the_recorded_launch(case):
    a, b = _run(case, True, True, "anneal"), _run(case, True, True, "late-change")
    for k in range(N_UPD):
        same = np.array_equal(a[f"td{k}"], b[f"td{k}"])
        assert same == (k < 5), (k, same)   # identical up to the change (update 5, behind the recording at update 3)
    _assert_same(a, _run(case, True, False, "anneal"), case)
    _assert_same(b, _run(case, True, False, "late-change"), case)


@pytest.mark.parametrize("setting", ["hipgraph-mode", "beta", "per", "two-members"])
def test_unsupported_combinations_stay_eager_and_run(setting):
    import super_sac_amd as ssa
    L = ssa.learning
    dev = torch.device("cuda")
    cfg = dict(CASES["sac_process" if setting == "beta" else "td3"], **({"E": 2} if setting == "two-members" else {}))
    old = L.LAUNCH_MODE
    L.LAUNCH_MODE = "graph" if setting == "hipgraph-mode" else old
    try:
        buf, agent, target, copt, eopt, las, aug, rp = _setup(ssa, cfg, dev, beta=setting == "beta")
        before = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()]).clone()
        for k in range(L.GRAPH_WARMUP + 2):
            rp.current_scale = 0.5 - 0.05 * k
            logs, dicts = _update(ssa, cfg, buf, agent, target, copt, eopt, las, aug, rp, per=setting == "per")
        after = torch.cat([p.detach().flatten() for p in agent.critics[0].parameters()])
        assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
        assert all(np.isfinite(float(v)) for v in logs.values())
        assert not agent.__dict__.get("_ssac_graphs") and not agent.__dict__.get("_ssac_fast")
    finally:
        L.LAUNCH_MODE = old


@pytest.mark.parametrize("case", ["td3", "sac_process"])
def test_a_noise_hook_that_comes_and_goes_records_again(case):
    """a stock recording, a hook installed before call 9 and removed before call 14: each change drops the recording
    (still_valid / drop_recording) and a new one, with the other noise source, serves the calls after"""
    import super_sac_amd as ssa
    n_upd, on, off = 20, 9, 14
    eager = _run(case, False, False, "anneal", hook_window=(on, off), n_upd=n_upd)
    rec = _run(case, False, True, "anneal", hook_window=(on, off), n_upd=n_upd)
    _assert_same(rec, eager, case)
    warm, steps = ssa.learning.GRAPH_WARMUP, rec["steps"]
    assert [s_[2] for s_ in steps] == [on - warm, on - warm + 1, off - warm, off - warm + 1, n_upd - warm]
    assert [s_[1] for s_ in steps] == [True, False, False, True, True]
    first, second, third = steps[0][0], steps[1][0], steps[3][0]
    assert steps[2][0] is second and steps[4][0] is third and len({id(first), id(second), id(third)}) == 3
    assert first.calls == on - warm - 1 and second.calls == off - on - 1 and third.calls == n_upd - off - 1
