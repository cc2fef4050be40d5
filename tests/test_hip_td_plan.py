"""GPU: learning_utils.compute_td_targets consumes exactly the host draws its plan lists (learning_utils.td_member_plan:
TdPlan.draws, then the REDQ subset) -- count, order and shape of the learning_utils.draw_normal / draw_subset calls and the
ticks of the agent's Philox stream, per head, with and without an exploration process, under the stock generator and
under a noise hook.  Values are pinned elsewhere (the fixture suite; tests/test_td_plan_cpu.py holds the plan to the
expressions it replaced): this file looks at what is consumed only.

Shapes: B 32 (two of the 16-row tiles), observation 5, hidden 32, 2 critics, subset 2, identity encoder, one member; A 2,
and once A 33 -- the tanh-normal head's 66 outputs are the smallest the fused kernels refuse (HEAD_MAX 64) at this
hidden size, so the per-layer path with a buffer draw runs on the device too."""
import copy
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
B, OBS, HIDDEN, N, N_SUB, ROWS = 32, 5, 32, 2, 2, 64
# (kind, process, stock generator) -> the plan's (head, launch, draws), worked out from the reference's draw order
# (learning_utils.py:322-338: head sample, then process noise) and the launch forms of DESIGN.md 4: a fused tanh-normal
# actor without a process samples in one launch, on the stream's tick while the generator is the stock one; head + process
# run as ssac_explore_action on that tick (the calls pass _explore as critic_update's verdict would), and keep the
# two-kernel sequence with buffer draws under a hook; a discrete update never looks at the process
EXPECTED = {
    ("stochastic", False, True): ("tanh_normal", "fused", ("tick",)),
    ("stochastic", False, False): ("tanh_normal", "fused", ("eps",)),
    ("stochastic", True, True): ("explore", "layers", ("tick",)),
    ("stochastic", True, False): ("tanh_normal", "layers", ("eps", "proc")),
    ("deterministic", False, True): ("deterministic", "layers", ()),
    ("deterministic", False, False): ("deterministic", "layers", ()),
    ("deterministic", True, True): ("explore", "layers", ("tick",)),
    ("deterministic", True, False): ("deterministic", "layers", ("proc",)),
    ("discrete", False, True): ("discrete", "layers", ()),
    ("discrete", False, False): ("discrete", "layers", ()),
    ("discrete", True, True): ("discrete", "layers", ()),
    ("discrete", True, False): ("discrete", "layers", ()),
}


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _setup(ssa, kind, A, dev, seed=11):
    torch.manual_seed(seed); np.random.seed(seed); random.seed(seed); torch.cuda.manual_seed(seed)
    discrete = kind == "discrete"
    buf = ssa.replay.ReplayBuffer(ROWS, device=dev)
    buf.load_experience(*synth.synth_transitions(ROWS, OBS, A, discrete, seed=seed + 100, n_actions=A))
    actor_cls = {"stochastic": ssa.nets.ContinuousStochasticActor, "deterministic": ssa.nets.ContinuousDeterministicActor,
                 "discrete": ssa.nets.DiscreteActor}[kind]
    agent = ssa.Agent(act_space_size=A, encoder=ssa.nets.IdentityEncoder(OBS), actor_network_cls=actor_cls,
                      critic_network_cls=ssa.nets.DiscreteCritic if discrete else ssa.nets.ContinuousCritic,
                      discrete=discrete, ensemble_size=1, num_critics=N, ucb_bonus=0.0, hidden_size=HIDDEN,
                      auto_rescale_targets=False)
    agent.to(dev)
    agent.train()
    target = copy.deepcopy(agent)
    la = torch.Tensor([math.log(0.1)]).to(dev)
    la.requires_grad = True
    aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])
    space = type("Space", (), {})()
    space.low, space.high = -np.ones(A, np.float32), np.ones(A, np.float32)
    rp = ssa.learning_utils.GaussianExplorationNoise(space, start_scale=0.3, final_scale=0.1, steps_annealed=1000)
    agent.__dict__["_ssac_noise"] = [0x5EED, 0, 0]
    ssa.learning_utils.ensure_adopted(agent, buf)
    ssa.learning_utils.ensure_adopted(target, buf)
    return buf, agent, target, [la], aug, rp


class _Watch:
    """logs the calls of learning_utils' two draw sites (which go on to draw) and the plans td_member_plan hands out;
    stock=False: a noise hook in rng.draw_normal / draw_normal_into (seeded host normals by call count)"""

    def __init__(self, ssa, mp, stock, dev):
        lu, self.events, self.plans = ssa.learning_utils, [], []
        draw_normal, draw_subset, plan = lu.draw_normal, lu.draw_subset, lu.td_member_plan
        if not stock:
            count = iter(range(1, 1 << 20))

            def normal(shape):
                return torch.randn(*shape, generator=torch.Generator().manual_seed(1000 + next(count)))
            mp.setattr(ssa.rng, "draw_normal", lambda shape, device: normal(shape).to(dev))
            mp.setattr(ssa.rng, "draw_normal_into", lambda dst: dst.copy_(normal(tuple(dst.shape))))
        assert ssa.rng.normal_is_stock() == stock
        mp.setattr(lu, "draw_normal", lambda shape, device: self.events.append(("normal", tuple(shape))) or draw_normal(shape, device))
        mp.setattr(lu, "draw_subset", lambda num, k: self.events.append(("subset", (num, k))) or draw_subset(num, k))
        mp.setattr(lu, "td_member_plan", lambda *a, **k: self.plans.append(plan(*a, **k)) or self.plans[-1])

    def check(self, ticks, A):
        """one compute_td_targets call happened: its events are its plan's draws, then the subset"""
        plan, = self.plans
        want = [("normal", (B, A)) for d in plan.draws if d in ("eps", "proc")] + [("subset", (N, N_SUB))]
        assert self.events == want, (plan, self.events)
        assert ticks == plan.draws.count("tick") and (plan.noise == "kernel") == (ticks == 1), (plan, ticks)
        assert not (ticks and len(want) > 1), "one source of noise per member"
        return plan


@pytest.mark.parametrize("stock", [True, False], ids=["stock", "hook"])
@pytest.mark.parametrize("process", [False, True], ids=["no-process", "process"])
@pytest.mark.parametrize("kind", ["stochastic", "deterministic", "discrete"])
def test_the_draws_of_a_call_are_its_plans(ssa, monkeypatch, kind, process, stock):
    lu, dev, A = ssa.learning_utils, torch.device("cuda"), 2
    buf, agent, target, las, aug, rp = _setup(ssa, kind, A, dev)
    rd = lu.sample_move_and_augment(buffer=buf, batch_size=B, augmenter=aug, aug_mix=0.0, per=False)
    watch = _Watch(ssa, monkeypatch, stock, dev)
    before = lu.noise_stream(agent, dev)[1]
    td, (s1_rep, a_s1) = lu.compute_td_targets(
        logs={}, replay_dict=rd, agent=agent, target_agent=target, ensemble_idx=0, ensemble_n=N_SUB, log_alphas=las,
        pop=False, gamma=0.99, random_process=rp if process else None, noise_clip=0.5, discrete=kind == "discrete",
        _explore=process and kind != "discrete")
    torch.cuda.synchronize()
    plan = watch.check(lu.noise_stream(agent, dev)[1] - before, A)
    assert (plan.head, plan.launch, plan.draws) == EXPECTED[kind, process, stock]
    assert td.shape == (B, 1) and bool(torch.isfinite(td).all()) and sorted(rd["_subset"]) == [0, 1]


def test_an_unfused_actor_draws_its_eps_from_a_buffer(ssa, monkeypatch):
    lu, dev, A = ssa.learning_utils, torch.device("cuda"), 33
    buf, agent, target, las, aug, rp = _setup(ssa, "stochastic", A, dev)
    narrow = ssa._lib.MlpDesc(0, 0, 1, OBS, HIDDEN, 64)
    wide = ssa._lib.MlpDesc(0, 0, 1, OBS, HIDDEN, 2 * A)
    import ctypes as C
    assert ssa._lib.lib.ssac_fused_supported(C.byref(narrow)) and not ssa._lib.lib.ssac_fused_supported(C.byref(wide))
    rd = lu.sample_move_and_augment(buffer=buf, batch_size=B, augmenter=aug, aug_mix=0.0, per=False)
    watch = _Watch(ssa, monkeypatch, True, dev)
    td, _ = lu.compute_td_targets(logs={}, replay_dict=rd, agent=agent, target_agent=target, ensemble_idx=0,
                                  ensemble_n=N_SUB, log_alphas=las, pop=False, gamma=0.99, random_process=None,
                                  noise_clip=None)
    torch.cuda.synchronize()
    plan = watch.check(lu.noise_stream(agent, dev)[1], A)
    assert (plan.head, plan.launch, plan.noise, plan.draws) == ("tanh_normal", "layers", "buffer", ("eps",))
    assert bool(torch.isfinite(td).all())


def test_the_chained_launch_takes_one_tick(ssa, monkeypatch):
    """the member's requests as learning._member_targets sets them (an eager critic_update): the actor sample is left
    pending and issued with the subset (TdPlan.launch "chain"), on one tick of the stream and no buffer draw"""
    L, lu, dev, A = ssa.learning, ssa.learning_utils, torch.device("cuda"), 2
    buf, agent, target, las, aug, rp = _setup(ssa, "stochastic", A, dev)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=3e-4, betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=1e-4)
    monkeypatch.setattr(L, "USE_GRAPHS", False)
    watch = _Watch(ssa, monkeypatch, True, dev)
    logs, dicts = L.critic_update(
        buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
        batch_size=B, gamma=0.99, critic_clip=None, encoder_clip=None, target_critic_ensemble_n=N_SUB,
        weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0, aug_mix=0.0,
        discrete=False, random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
    torch.cuda.synchronize()
    plan = watch.check(lu.noise_stream(agent, dev)[1], A)
    assert (plan.head, plan.launch, plan.draws) == ("tanh_normal", "chain", ("tick",))
    assert all(math.isfinite(float(v)) for v in logs.values()) and bool(torch.isfinite(dicts[0]["td_target"]).all())
