"""GPU: acting with a plain conv-stack encoder (MinAtar's) on uint8 frames: forward and sample_action take the recorded
plan (acting._PLANS), and equal the general path -- logits within the project's ATOL_GENERAL = 2e-5 (both paths run the same
kernels; the recorded one reads the frames from the plan's observation buffer), greedy actions equal on every row whose
top-two logit gap exceeds 4 x that, Python's ``random`` stream consumed alike."""
import random

import numpy as np
import pytest
import torch

import conv_stack_cases as cc

pytestmark = pytest.mark.gpu

ATOL_GENERAL = 2e-5   # tests/test_hip_acting_fast.py::test_pixel_agents_take_the_one_call_path_and_equal_the_general_path
CFG = cc.CONFIGS["minatar"]
OWN = pytest.mark.parametrize("own", [False, True], ids=["adopted", "ssa.nets.ConvStackEncoder"])
FORMS = pytest.mark.parametrize("form", ["all", False], ids=["fused", "layers"])


@pytest.fixture
def launch_form(form):
    from super_sac_amd import conv_encoder as ce
    saved = ce.STACK_FUSED
    ce.STACK_FUSED = form
    yield form
    ce.STACK_FUSED = saved


def _agent(own):
    import ssac_oracle
    agent = cc.runner.engine_agent(ssac_oracle, CFG, torch.device("cuda"), own)
    agent.__dict__["_ssac_noise"] = [4321, 0, 0]
    return agent


def _frames(n, seed, count):
    rs = np.random.RandomState(seed)
    shape = CFG["obs"] if n == 1 else (n,) + CFG["obs"]
    return [(rs.uniform(size=shape) < 0.3).astype(np.uint8) for _ in range(count)]


def _general(fn):
    """fn() with the recorded path switched off"""
    from super_sac_amd import acting
    acting.ENABLED = False
    try:
        return fn()
    finally:
        acting.ENABLED = True


@pytest.mark.parametrize("n", [1, 4])
@OWN
@FORMS
def test_forward_and_sample_action_take_the_plan_and_equal_the_general_path(launch_form, own, n):
    from super_sac_amd import acting
    agent = _agent(own)
    for obs in _frames(n, 40 + n, 3):
        random.seed(5)
        fast = agent.forward({"obs": obs}, num_envs=n)
        fast_act, logits = agent.sample_action({"obs": obs}, num_envs=n, return_dist=True)
        fast_state = random.getstate()
        plans = acting._PLANS.get(agent, {})
        assert ("forward", n, 0.0) in plans and ("sample", n, 0.0) in plans, "the calls did not take the recorded path"
        assert plans[("forward", n, 0.0)].pixel_shape == CFG["obs"]
        random.seed(5)
        want = _general(lambda: agent.forward({"obs": obs}, num_envs=n))
        _, want_logits = _general(lambda: agent.sample_action({"obs": obs}, num_envs=n, return_dist=True))
        assert random.getstate() == fast_state, "the recorded path consumed Python's random stream differently"
        assert fast.shape == want.shape and fast.dtype == want.dtype and np.asarray(fast_act).shape == np.asarray(want).shape
        got, ref = logits.detach().cpu().numpy().reshape(n, -1), want_logits.detach().cpu().numpy().reshape(n, -1)
        print(f"n={n} logits: max deviation {np.abs(got - ref).max():.3e}")
        np.testing.assert_allclose(got, ref, atol=ATOL_GENERAL, rtol=0)
        top = np.sort(ref, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 4 * ATOL_GENERAL
        assert clear.any()
        assert np.array_equal(np.asarray(fast).reshape(n, -1)[clear], np.asarray(want).reshape(n, -1)[clear])


@OWN
def test_the_plan_computes_the_reference_arithmetic(own):
    """greedy actions of the recorded plan = argmax of the oracle's actor on the oracle's encoding of the RAW frames (the
    parent fed x / 255 into conv1)"""
    import ssac_oracle as orc
    from super_sac_amd import acting
    n = 4
    agent = _agent(own)
    oa = cc.runner.oracle_agent(orc, CFG, torch.float64)
    encode = cc.patched_encode(orc)
    for obs in _frames(n, 77, 2):
        fast = agent.forward({"obs": obs}, num_envs=n)
        assert ("forward", n, 0.0) in acting._PLANS.get(agent, {})
        rep = encode(oa.encoder, {"obs": torch.from_numpy(obs)})
        want = orc.mlp3(oa.actors[0], rep)[0]
        top = torch.sort(want, dim=1).values
        clear = ((top[:, -1] - top[:, -2]) > 1e-4).numpy()
        assert clear.any()
        assert np.array_equal(np.asarray(fast).reshape(n)[clear], want.argmax(1).numpy()[clear])
