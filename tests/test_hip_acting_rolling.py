"""GPU: the recorded acting path (super_sac_amd/acting.py) under the training loop's defaults -- rolling=True calls of pixel
agents whose encoder's rolling interface is the inherited pass-through -- and for float32 frame observations
(csrc/ssac_act.hip: ssac_act_ingest_f32 in front of the recorded encoder launches).  The float32 plans are switched on by
`acting.FLOAT32_FRAMES = True`; its default is off, because float frames on the general path is what
tests/test_hip_acting_fast.py::test_ineligible_calls_take_the_general_path pins for a caller who asked for nothing.

Pinning, as profiles/acting_rules.md describes it: the agent's noise seed (`_ssac_noise`) and the plans' stream serial
(`acting._SERIAL`) fixed, Python's `random` seeded for the host draw of the acting actor.

Tolerance between the recorded and the general path for pixel agents: ATOL_GENERAL = 2e-5 on the actors' head outputs and
equal greedy actions, the constants of tests/test_hip_acting_fast.py::
test_pixel_agents_take_the_one_call_path_and_equal_the_general_path (the recorded path gathers the first layer's patches
from the frames itself; the general path converts the frames to a float tensor first).  A continuous greedy action is the
mean of tanh of head outputs (|tanh'| <= 1): the same bound holds for it."""
import random

import numpy as np
import pytest
import torch

import case_runner
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE_SEED = 0x0A11CE5EED0F5EED
ATOL_GENERAL = 2e-5   # tests/test_hip_acting_fast.py::test_pixel_agents_take_the_one_call_path_and_equal_the_general_path

ATARI = synth.CASES["atari_pixels"]                                          # SmallPixelEncoder, 4 x 84 x 84, discrete, E = 1
DRQ = synth.CASES["drqv2_pixels"]                                            # BigPixelEncoder, 9 x 84 x 84, deterministic actor
DRQ_STOCHASTIC = dict(DRQ, actor="stochastic")                               # ... with a tanh-normal head: the sample draws noise
ATARI_SUNRISE = dict(ATARI, E=3, weight_type="sunrise", temp=20.0)           # 3 members x 2 critics: the UCB rule, the host draw

# (case, rule, ucb bonus): forward, continuous sample, discrete sample, discrete greedy, discrete UCB
RULES = [("drq", DRQ, "forward", 0.0), ("drq_stochastic", DRQ_STOCHASTIC, "sample", 0.0), ("atari", ATARI, "sample", 0.0),
         ("atari", ATARI, "forward", 0.0), ("atari_sunrise", ATARI_SUNRISE, "sample", 0.7)]


def _agent(cfg, ucb=0.0):
    agent = case_runner.build_engine_agent(cfg, torch.device(DEV))
    agent.ucb_bonus = ucb
    agent.__dict__["_ssac_noise"] = [NOISE_SEED, 0, 0]
    return agent


def _frames(cfg, n, seed, count=1):
    px = cfg["pixels"]
    rs = np.random.RandomState(seed)
    shape = (px["channels"], px["hw"], px["hw"])
    return [rs.randint(0, 256, ((n,) + shape) if n > 1 else shape).astype(np.uint8) for _ in range(count)]


def _call(agent, rule, obs, n, rolling, return_dist=False):
    if rule == "forward":
        return agent.forward({"obs": obs}, num_envs=n, rolling=rolling)
    return agent.sample_action({"obs": obs}, num_envs=n, rolling=rolling, return_dist=return_dist)


def _general(fn):
    """fn() with the recorded path switched off"""
    from super_sac_amd import acting
    acting.ENABLED = False
    try:
        return fn()
    finally:
        acting.ENABLED = True


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cfg", [ATARI, DRQ], ids=["atari", "drq"])
def test_rolling_calls_record_a_plan(cfg, n):
    """1. forward / sample_action with rolling=True (what main.super_sac and evaluation.run_env pass) on a pixel agent"""
    from super_sac_amd import acting
    agent = _agent(cfg)
    obs = _frames(cfg, n, 11)[0]
    assert acting._eligible(agent, {"obs": obs}, n, False, True) and acting._eligible(agent, {"obs": obs}, n, True, True)
    agent.forward({"obs": obs}, num_envs=n, rolling=True)
    agent.sample_action({"obs": obs}, num_envs=n, rolling=True)
    plans = acting._PLANS.get(agent, {})
    assert ("forward", n, 0.0) in plans and ("sample", n, 0.0) in plans
    px = cfg["pixels"]
    assert plans[("forward", n, 0.0)].pixel_shape == (px["channels"], px["hw"], px["hw"])
    # the plan is not keyed on `rolling`: a rolling=False call is served by the same plan
    plan = plans[("forward", n, 0.0)]
    agent.forward({"obs": obs}, num_envs=n, rolling=False)
    assert acting._PLANS[agent][("forward", n, 0.0)] is plan and len(acting._PLANS[agent]) == 2


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,cfg,rule,ucb", RULES, ids=[f"{r[0]}-{r[2]}" + ("-ucb" if r[3] else "") for r in RULES])
def test_rolling_true_returns_the_bytes_of_rolling_false(name, cfg, rule, ucb, n, monkeypatch):
    """2. five calls with rolling=True against five with rolling=False on a fresh copy of the agent: same noise seed, same plan
    serial, same host draws -- the same bytes (actions and, for the sampling rules, the logged head output)"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [8000 + n])
    frames = _frames(cfg, n, 21 + n, count=5)
    got = {}
    for rolling in (True, False):
        acting._SERIAL[0] = 8000 + n
        agent = _agent(cfg, ucb)
        random.seed(77)
        outs = []
        for obs in frames:
            r = _call(agent, rule, obs, n, rolling, return_dist=rule == "sample")
            outs.append(r if rule == "forward" else (r[0], r[1].cpu().numpy()))
        pkey = (rule, n, float(ucb))
        assert pkey in acting._PLANS.get(agent, {}), "the call did not take the recorded path"
        got[rolling] = outs
    for a, b in zip(got[True], got[False]):
        if rule == "forward":
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        else:
            assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    if name == "drq_stochastic":   # (the noise is really there: five draws, five different actions on five different frames)
        assert len({a[0].tobytes() for a in got[True]}) == 5


@pytest.mark.parametrize("n", [1, 3])
def test_rolling_true_equals_the_general_path(n):
    """3. the deterministic rules -- forward (continuous) and discrete greedy -- with rolling=True on both paths; the discrete
    agent's logits (the logged head output of its single actor) within ATOL_GENERAL"""
    from super_sac_amd import acting
    for cfg in (DRQ, ATARI):
        agent = _agent(cfg)
        for obs in _frames(cfg, n, 31 + n, count=2):
            fast = agent.forward({"obs": obs}, num_envs=n, rolling=True)
            assert ("forward", n, 0.0) in acting._PLANS.get(agent, {})
            want = _general(lambda: agent.forward({"obs": obs}, num_envs=n, rolling=True))
            assert fast.shape == want.shape and fast.dtype == want.dtype
            if cfg["discrete"]:
                assert np.array_equal(fast, want)
                _, logits = agent.sample_action({"obs": obs}, num_envs=n, rolling=True, return_dist=True)
                _, want_logits = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, rolling=True, return_dist=True))
                print(f"n={n} logits: max deviation {float((logits - want_logits).abs().max()):.3e}")
                np.testing.assert_allclose(logits.cpu().numpy(), want_logits.cpu().numpy(), atol=ATOL_GENERAL, rtol=0)
            else:
                print(f"n={n} continuous forward: max deviation {float(np.abs(fast - want).max()):.3e}")
                np.testing.assert_allclose(fast, want, atol=ATOL_GENERAL, rtol=0)


def test_stateful_encoders_stay_on_the_general_path():
    """4. an encoder that overrides forward_rolling (it counts its calls) and one that overrides only reset_rolling: declined
    under rolling=True, served by the general path, still recorded under rolling=False"""
    import super_sac_amd as ssa
    from super_sac_amd import acting

    class Counting(ssa.nets.PixelEncoder):
        def forward_rolling(self, obs):
            self.__dict__["rolled"] = self.__dict__.get("rolled", 0) + 1
            return self.forward(obs)

    class Resetting(ssa.nets.PixelEncoder):
        def reset_rolling(self):
            self.__dict__["resets"] = self.__dict__.get("resets", 0) + 1

    n = 3
    for cls in (Counting, Resetting):
        agent = _agent(ATARI)
        agent.encoder.__class__ = cls          # (the same parameters under the subclass; nothing was asked of the encoder yet)
        frames = _frames(ATARI, n, 41, count=3)
        rolled = lambda: agent.encoder.__dict__.get("rolled", 0)
        for step, obs in enumerate(frames):
            assert not acting._eligible(agent, {"obs": obs}, n, False, True)
            assert not acting._eligible(agent, {"obs": obs}, n, True, True)
            before = rolled()
            greedy = agent.forward({"obs": obs}, num_envs=n, rolling=True)
            assert cls is not Counting or rolled() == before + 1          # once per step
            torch.manual_seed(900 + step); random.seed(900 + step)
            act = agent.sample_action({"obs": obs}, num_envs=n, rolling=True)
            assert cls is not Counting or rolled() == before + 2
            assert agent not in acting._PLANS
            want_greedy = _general(lambda: agent.forward({"obs": obs}, num_envs=n, rolling=True))
            torch.manual_seed(900 + step); random.seed(900 + step)
            want_act = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, rolling=True))
            assert np.array_equal(greedy, want_greedy) and np.array_equal(act, want_act)
        obs = frames[0]
        assert acting._eligible(agent, {"obs": obs}, n, False, False)
        before = rolled()
        greedy = agent.forward({"obs": obs}, num_envs=n, rolling=False)
        assert ("forward", n, 0.0) in acting._PLANS[agent] and rolled() == before
        assert np.array_equal(greedy, _general(lambda: agent.forward({"obs": obs}, num_envs=n, rolling=False)))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cfg", [ATARI, DRQ_STOCHASTIC], ids=["atari", "drq_stochastic"])
def test_float32_frames_return_the_bytes_of_the_uint8_plan(cfg, n, monkeypatch):
    """5. integer-valued float32 frames: forward, and sample on a pinned stream (the two plans get the same serial and make the
    same number of calls), byte for byte the uint8 plan's answers; both plans live side by side; the frames are not written"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "FLOAT32_FRAMES", True, raising=False)
    monkeypatch.setattr(acting, "_SERIAL", [8100 + n])
    agent = _agent(cfg)
    frames = _frames(cfg, n, 51 + n, count=3)
    got = {}
    for dtype in (np.uint8, np.float32):
        acting._SERIAL[0] = 8100 + n
        random.seed(78)
        outs = []
        for obs in frames:
            v = obs.astype(dtype)
            keep = v.copy()
            v.flags.writeable = False
            assert acting._eligible(agent, {"obs": v}, n, True, True)
            greedy = agent.forward({"obs": v}, num_envs=n, rolling=True)
            act, dist = agent.sample_action({"obs": v}, num_envs=n, rolling=True, return_dist=True)
            assert np.array_equal(v, keep)
            outs.append((greedy, act, dist.cpu().numpy()))
        got[dtype] = outs
    plans = acting._PLANS[agent]
    assert set(plans) == {("forward", n, 0.0), ("sample", n, 0.0), ("forward", n, 0.0, "float32"), ("sample", n, 0.0, "float32")}
    assert plans[("forward", n, 0.0)].obs_dtype == np.uint8 and plans[("forward", n, 0.0, "float32")].obs_dtype == np.float32
    assert plans[("sample", n, 0.0)].serial == plans[("sample", n, 0.0, "float32")].serial
    for a, b in zip(got[np.uint8], got[np.float32]):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    if not cfg["discrete"]:
        assert len({a[1].tobytes() for a in got[np.float32]}) == 3   # (noise drawn: three frames, three actions)


@pytest.mark.parametrize("n", [1, 3])
def test_fractional_float32_frames_equal_the_general_path(n, monkeypatch):
    """5. frames with fractional values (x + 0.25): nothing is rounded on the way -- against the general path on the same
    frames within ATOL_GENERAL"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "FLOAT32_FRAMES", True, raising=False)
    for cfg in (DRQ, ATARI):
        agent = _agent(cfg)
        obs = _frames(cfg, n, 61 + n)[0].astype(np.float32) + np.float32(0.25)
        fast = agent.forward({"obs": obs}, num_envs=n, rolling=True)
        assert ("forward", n, 0.0, "float32") in acting._PLANS.get(agent, {})
        want = _general(lambda: agent.forward({"obs": obs}, num_envs=n, rolling=True))
        if cfg["discrete"]:
            assert np.array_equal(fast, want)
            _, logits = agent.sample_action({"obs": obs}, num_envs=n, rolling=True, return_dist=True)
            _, want_logits = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, rolling=True, return_dist=True))
            print(f"n={n} logits: max deviation {float((logits - want_logits).abs().max()):.3e}")
            np.testing.assert_allclose(logits.cpu().numpy(), want_logits.cpu().numpy(), atol=ATOL_GENERAL, rtol=0)
            # ... and the fraction is seen: the uint8 frames give other logits
            _, floor_logits = agent.sample_action({"obs": obs.astype(np.uint8)}, num_envs=n, rolling=True, return_dist=True)
            assert not torch.equal(floor_logits, logits)
        else:
            print(f"n={n} continuous forward: max deviation {float(np.abs(fast - want).max()):.3e}")
            np.testing.assert_allclose(fast, want, atol=ATOL_GENERAL, rtol=0)


def test_ingest_kernel_alone_at_a_size_that_is_no_multiple_of_four():
    """5. synth's Atari-style encoder is built for 84 x 84 frames only (an odd width is not accepted), so: the ingest kernel
    through its C entry point at (3, 7, 9) -- 189 floats: 47 vectors of 16 bytes and a tail of one -- and at every tail length,
    exact against numpy.astype; nothing behind the last float is written, the source is not written; bad arguments are
    refused before any launch"""
    from super_sac_amd._lib import check, lib
    st = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(71)
    for shape in ((3, 7, 9), (1, 2, 3), (2, 2, 2), (2, 5, 1), (3, 37, 37), (3, 701, 701)):
        # 189, 6, 8, 10, 4107 and 1474203 floats (the last: more vectors than the launch has lanes -- the grid-stride loop)
        frames = (rs.randint(0, 256, shape).astype(np.float64) + rs.choice([0.0, 0.25, 0.5], shape))
        n = frames.size
        src = torch.from_numpy(frames.astype(np.float32)).to(DEV)
        src_before = src.clone()
        dst = torch.full((n + 64,), -7.0, device=DEV)
        check(lib.ssac_act_ingest_f32(src.data_ptr(), dst.data_ptr(), n, st))
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        assert out[:n].tobytes() == frames.astype(np.float32).reshape(-1).tobytes(), shape
        assert np.all(out[n:] == -7.0), shape
        assert torch.equal(src, src_before)
    src, dst = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    assert lib.ssac_act_ingest_f32(src.data_ptr() + 4, dst.data_ptr(), 8, st) != 0      # (a source off the 16-byte grid)
    assert lib.ssac_act_ingest_f32(src.data_ptr(), dst.data_ptr() + 8, 8, st) != 0
    assert lib.ssac_act_ingest_f32(src.data_ptr(), dst.data_ptr(), 0, st) != 0
    assert lib.ssac_act_ingest_f32(None, dst.data_ptr(), 8, st) != 0
    assert b"ssac_act_ingest_f32" in lib.ssac_last_error()


@pytest.mark.parametrize("n", [1, 3])
def test_float32_frames_of_an_odd_width_through_a_plan(n, monkeypatch):
    """5. ... and end to end on an agent built here around the package's Atari-style encoder at 3 x 37 x 37 (the smallest odd
    square it takes; 4107 floats per frame: a tail of 3 at n = 1, of 1 at n = 3): float32 frames return the bytes of the uint8
    plan, fractional ones the general path's action within ATOL_GENERAL"""
    import super_sac_amd as ssa
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "FLOAT32_FRAMES", True, raising=False)
    monkeypatch.setattr(acting, "_SERIAL", [8200 + n])
    torch.manual_seed(8)
    enc = ssa.nets.PixelEncoder(ssa.nets.SmallPixelEncoder((3, 37, 37), 32))
    agent = ssa.Agent(act_space_size=3, encoder=enc, actor_network_cls=ssa.nets.ContinuousStochasticActor,
                      critic_network_cls=ssa.nets.ContinuousCritic, discrete=False, ensemble_size=2, num_critics=2,
                      hidden_size=64, auto_rescale_targets=False)
    agent.to(torch.device(DEV))
    agent.__dict__["_ssac_noise"] = [NOISE_SEED, 0, 0]
    rs = np.random.RandomState(81 + n)
    obs = rs.randint(0, 256, (n, 3, 37, 37) if n > 1 else (3, 37, 37)).astype(np.uint8)
    assert (obs.size * 4) % 16 != 0
    got = {}
    for dtype in (np.uint8, np.float32):
        acting._SERIAL[0] = 8200 + n
        random.seed(79)
        v = obs.astype(dtype)
        got[dtype] = (agent.forward({"obs": v}, num_envs=n, rolling=True),
                      agent.sample_action({"obs": v}, num_envs=n, rolling=True))
    assert ("forward", n, 0.0, "float32") in acting._PLANS[agent] and ("sample", n, 0.0, "float32") in acting._PLANS[agent]
    for x, y in zip(got[np.uint8], got[np.float32]):
        assert x.shape == ((n, 3) if n > 1 else (3,)) and x.tobytes() == y.tobytes()
    frac = obs.astype(np.float32) + np.float32(0.25)
    fast = agent.forward({"obs": frac}, num_envs=n, rolling=True)
    want = _general(lambda: agent.forward({"obs": frac}, num_envs=n, rolling=True))
    print(f"n={n} 3x37x37 forward: max deviation {float(np.abs(fast - want).max()):.3e}")
    np.testing.assert_allclose(fast, want, atol=ATOL_GENERAL, rtol=0)
    assert not np.array_equal(fast, got[np.float32][0])


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ucb", [0.0, 0.7])
def test_host_rng_contract_under_rolling(ucb, monkeypatch):
    """6. the reference's host draws -- random.choice(self.actors), under UCB random.choice(act_dists) -- are consumed by the
    recorded path under rolling=True exactly as by the general path: the same generator state after N calls"""
    from super_sac_amd import acting
    monkeypatch.setattr(acting, "_SERIAL", [8300])
    agent = _agent(ATARI_SUNRISE, ucb)
    frames = _frames(ATARI_SUNRISE, 1, 91, count=6)
    random.seed(4242)
    start = random.getstate()
    for obs in frames:
        agent.forward({"obs": obs}, rolling=True)
        agent.sample_action({"obs": obs}, rolling=True)
    fast_state = random.getstate()
    assert ("sample", 1, float(ucb)) in acting._PLANS[agent] and fast_state != start
    random.seed(4242)

    def general():
        for obs in frames:
            agent.forward({"obs": obs}, rolling=True)
            agent.sample_action({"obs": obs}, rolling=True)
    _general(general)
    assert random.getstate() == fast_state


def test_what_is_still_declined_under_rolling(monkeypatch):
    """7. float64 (and integer, and half) frames, Beta actors and an injected-noise hook: `_eligible` says no with rolling=True
    as with rolling=False (what tests/test_hip_acting_fast.py, test_hip_acting.py and test_hip_beta.py pin, restated) -- and so
    do float32 frames while FLOAT32_FRAMES is at its default"""
    import super_sac_amd as ssa
    from super_sac_amd import acting
    agent = _agent(ATARI)
    obs = _frames(ATARI, 1, 95)[0]
    assert acting.FLOAT32_FRAMES is False
    for rolling in (False, True):
        assert not acting._eligible(agent, {"obs": obs.astype(np.float32)}, 1, True, rolling)
    act = agent.sample_action({"obs": obs.astype(np.float32)}, rolling=True)
    assert act.shape == (1,) and agent not in acting._PLANS
    monkeypatch.setattr(acting, "FLOAT32_FRAMES", True)
    assert acting._eligible(agent, {"obs": obs.astype(np.float32)}, 1, True, True)
    for dtype in (np.float64, np.float16, np.int32, np.int8):
        for sample in (False, True):
            assert not acting._eligible(agent, {"obs": obs.astype(dtype)}, 1, sample, True)
    act = agent.sample_action({"obs": obs.astype(np.float64)}, rolling=True)
    assert act.shape == (1,) and agent not in acting._PLANS
    # wrong sizes and channel counts of float32 frames
    assert not acting._eligible(agent, {"obs": obs.astype(np.float32)[:3]}, 1, False, True)
    assert not acting._eligible(agent, {"obs": obs.astype(np.float32)}, 2, False, True)
    # an injected-noise hook: the sample of a tanh-normal head goes through it
    agent = _agent(DRQ_STOCHASTIC)
    obs = _frames(DRQ, 1, 96)[0]
    assert acting._eligible(agent, {"obs": obs}, 1, True, True)
    saved = ssa.rng.draw_normal
    ssa.rng.draw_normal = lambda shape, device: torch.zeros(shape, device=device)
    try:
        for v in (obs, obs.astype(np.float32)):
            assert not acting._eligible(agent, {"obs": v}, 1, True, True)
    finally:
        ssa.rng.draw_normal = saved
    # Beta actors on a pixel encoder
    torch.manual_seed(9)
    enc = ssa.nets.PixelEncoder(ssa.nets.SmallPixelEncoder((4, 84, 84), 32))
    beta = ssa.Agent(act_space_size=3, encoder=enc, actor_network_cls=ssa.nets.ContinuousStochasticActor,
                     critic_network_cls=ssa.nets.ContinuousCritic, discrete=False, ensemble_size=1, num_critics=2,
                     hidden_size=64, auto_rescale_targets=False, beta_dist=True)
    beta.to(torch.device(DEV))
    obs = _frames(ATARI, 1, 97)[0]
    for v in (obs, obs.astype(np.float32)):
        for sample in (False, True):
            assert not acting._eligible(beta, {"obs": v}, 1, sample, True)
            assert not acting._eligible(beta, {"obs": v}, 1, sample, False)
