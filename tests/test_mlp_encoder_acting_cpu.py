"""CPU: which calls of an agent with a two-layer MLP encoder the acting path records (super_sac_amd/acting.py: _mlp_obs,
_eligible, _plan_key, _signature).  Nothing here launches a kernel: eligibility, the plan key and the signature are host
decisions, and recognising an encoder on its first acting call probes it with a local generator."""
import copy
import random

import numpy as np
import pytest
import torch
from torch import nn
import torch.nn.functional as F

import mlp_encoder_cases as mc

CPU = torch.device("cpu")
KINDS = [("sac", False), ("sac", True), ("visgrid", False), ("visgrid", True)]
IDS = ["SharedEncoderLike", "MlpEncoder-vector", "VisgridEncoderLike", "MlpEncoder-grid"]


def _agent(name, own):
    import ssac_oracle as orc
    return mc.engine_agent(orc, mc.CONFIGS[name], CPU, own)


def _obs(name, n, dtype=np.float32, seed=0):
    shape = mc.CONFIGS[name]["obs"]
    return {"obs": np.random.RandomState(seed).standard_normal(shape if n == 1 else (n,) + shape).astype(dtype)}


@pytest.mark.parametrize("name,own", KINDS, ids=IDS)
def test_a_recognised_mlp_encoder_and_an_observation_of_the_right_size_are_eligible(name, own):
    from super_sac_amd import acting, mlp_encoder
    agent = _agent(name, own)
    assert not mlp_encoder.is_mlp_encoder(agent.encoder)        # nobody has looked at it yet
    for n in (1, 4):
        for sample in (False, True):
            assert acting._eligible(agent, _obs(name, n), n, sample, False)
    assert mlp_encoder.is_mlp_encoder(agent.encoder)
    K = int(np.prod(mc.CONFIGS[name]["obs"]))
    assert acting._mlp_obs(agent, _obs(name, 4), 4) == ("obs", K)
    # any shape with the right element count, any dtype that converts to float32 (the identity plan's rule)
    flat = {"obs": _obs(name, 4)["obs"].reshape(-1)}
    assert acting._eligible(agent, flat, 4, False, False)
    assert acting._eligible(agent, _obs(name, 4, np.float64), 4, True, False)


@pytest.mark.parametrize("name,own", KINDS, ids=IDS)
def test_a_wrong_element_count_is_not_eligible(name, own):
    from super_sac_amd import acting
    agent = _agent(name, own)
    assert acting._eligible(agent, _obs(name, 4), 4, False, False)
    assert not acting._eligible(agent, _obs(name, 4), 3, False, False)
    assert not acting._eligible(agent, _obs(name, 1), 4, True, False)
    assert not acting._eligible(agent, {"obs": np.zeros((4, 5), np.float32)}, 4, False, False)
    assert not acting._eligible(agent, {"other": _obs(name, 4)["obs"]}, 4, False, False)
    assert not acting._eligible(agent, {"obs": torch.zeros(4, 11)}, 4, False, False)   # (tensors: the general path)


def test_rolling_follows_the_pixel_rule():
    import super_sac_amd as ssa
    from super_sac_amd import acting
    agent = _agent("sac", True)          # ssa.nets.MlpEncoder inherits the pass-through rolling interface
    assert acting._eligible(agent, _obs("sac", 4), 4, True, True)

    class Stateful(ssa.nets.MlpEncoder):
        def forward_rolling(self, obs):
            return self.forward(obs)
    cfg = mc.CONFIGS["sac"]
    agent.encoder = Stateful(cfg["obs"], cfg["enc_hidden"], cfg["emb"], out_act=cfg["enc_act"])
    assert acting._eligible(agent, _obs("sac", 4), 4, True, False)
    assert not acting._eligible(agent, _obs("sac", 4), 4, True, True)
    # the stand-ins define the interface themselves (no Encoder base of the reference's module and name): stateful for all
    # the detection can tell
    standin = _agent("sac", False)
    assert acting._eligible(standin, _obs("sac", 4), 4, False, False)
    assert not acting._eligible(standin, _obs("sac", 4), 4, False, True)


class _ThreeLinears(nn.Module):
    def __init__(self, dim=11):
        super().__init__()
        self.have_at_least_one_param = nn.Linear(1, 1)
        self.a, self.b, self.c = nn.Linear(dim, 32), nn.Linear(32, 32), nn.Linear(32, dim)
        self._dim = dim

    @property
    def embedding_dim(self):
        return self._dim

    def forward(self, o):
        return F.relu(self.c(F.relu(self.b(F.relu(self.a(o["obs"]))))))


def test_a_module_the_recogniser_refuses_is_not_eligible():
    from super_sac_amd import acting, mlp_encoder
    agent = _agent("sac", False)
    agent.encoder = _ThreeLinears(11)
    assert not acting._eligible(agent, _obs("sac", 4), 4, False, False)
    assert not acting._eligible(agent, _obs("sac", 1), 1, True, False)
    assert not mlp_encoder.is_mlp_encoder(agent.encoder)


def test_agents_the_updates_refuse_stay_on_the_general_path():
    from super_sac_amd import acting
    agent = _agent("sac", True)
    assert acting._eligible(agent, _obs("sac", 4), 4, False, False)
    agent.actors[0].__dict__["_ssac_precision"] = "bf16"
    assert not acting._eligible(agent, _obs("sac", 4), 4, False, False)
    del agent.actors[0].__dict__["_ssac_precision"]
    assert acting._eligible(agent, _obs("sac", 4), 4, False, False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_the_plan_key_has_no_dtype_suffix(dtype):
    from super_sac_amd import acting
    agent = _agent("sac", True)
    for n in (1, 4):
        obs = _obs("sac", n, dtype)
        assert acting._eligible(agent, obs, n, True, False)
        assert acting._plan_key(agent, obs, n, False) == ("forward", False, ("forward", n, 0.0))
        assert acting._plan_key(agent, obs, n, True) == ("sample", False, ("sample", n, 0.0))
    ens = _agent("ensemble", True)
    ens.ucb_bonus = 0.7
    obs = _obs("ensemble", 6, dtype)
    assert acting._eligible(ens, obs, 6, True, False)
    assert acting._plan_key(ens, obs, 6, True) == ("ucb", True, ("sample" if ens.discrete else "ucb", 6, 0.7))


@pytest.mark.parametrize("own", [False, True], ids=["adopted", "ssa.nets.MlpEncoder"])
def test_the_signature_follows_the_first_layer_weight(own):
    from super_sac_amd import acting
    agent = _agent("sac", own)
    assert acting._eligible(agent, _obs("sac", 4), 4, False, False)
    sig = acting._signature(agent, False)
    lin0 = agent.encoder.__dict__["_ssac_mlp_desc"][0]
    assert lin0.weight.data_ptr() in sig
    assert acting._signature(agent, False) == sig
    agent.encoder = copy.deepcopy(agent.encoder)
    assert acting._eligible(agent, _obs("sac", 4), 4, False, False)
    assert acting._signature(agent, False) != sig


@pytest.mark.parametrize("name,own", KINDS, ids=IDS)
def test_recognition_on_first_contact_moves_no_global_random_stream(name, own):
    from super_sac_amd import acting, mlp_encoder
    agent = _agent(name, own)
    obs = _obs(name, 4)
    torch.manual_seed(7); np.random.seed(7); random.seed(7)
    t0, n0, p0 = torch.get_rng_state(), np.random.get_state(), random.getstate()
    assert not mlp_encoder.is_mlp_encoder(agent.encoder)
    assert acting._eligible(agent, obs, 4, True, False)
    assert mlp_encoder.is_mlp_encoder(agent.encoder)
    assert torch.equal(torch.get_rng_state(), t0) and random.getstate() == p0
    n1 = np.random.get_state()
    assert n1[0] == n0[0] and np.array_equal(n1[1], n0[1]) and n1[2:] == n0[2:]
