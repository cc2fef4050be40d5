"""CPU: recognition of two-layer MLP encoders (super_sac_amd/mlp_encoder.py), the arena layout and its binding."""
import copy
import random

import numpy as np
import pytest
import torch
from torch import nn
import torch.nn.functional as F

import mlp_encoder_cases as mc
import super_sac_amd as ssa
from super_sac_amd import learning_utils as lu
from super_sac_amd import mlp_encoder as me

REFUSAL = "this encoder has no HIP path"


def _obs(shape=(11,), rows=3, key="obs"):
    return {key: torch.zeros((rows,) + shape)}


class _Base(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.have_at_least_one_param = nn.Linear(1, 1)
        self._dim = dim

    @property
    def embedding_dim(self):
        return self._dim


class ThreeLinears(_Base):
    def __init__(self, dim=11):
        super().__init__(dim)
        self.a, self.b, self.c = nn.Linear(dim, 32), nn.Linear(32, 32), nn.Linear(32, dim)

    def forward(self, o):
        return F.relu(self.c(F.relu(self.b(F.relu(self.a(o["obs"]))))))


class TanhHidden(_Base):
    def __init__(self, dim=11):
        super().__init__(dim)
        self.a, self.b = nn.Linear(dim, 32), nn.Linear(32, dim)

    def forward(self, o):
        return F.relu(self.b(torch.tanh(self.a(o["obs"]))))


class NormBetween(_Base):
    def __init__(self, dim=11):
        super().__init__(dim)
        self.a, self.n, self.b = nn.Linear(dim, 32), nn.LayerNorm(32), nn.Linear(32, dim)

    def forward(self, o):
        return F.relu(self.b(F.relu(self.n(self.a(o["obs"])))))


def test_recognition_accepts_the_stand_ins_and_the_package_class():
    enc = mc.SharedEncoderLike(11, 64)
    lin0, lin1, act2, key = me.find_mlp_encoder(enc, _obs())
    assert (lin0, lin1, act2, key) == (enc.fc0, enc.fc1, "relu", "obs")
    vis = mc.VisgridEncoderLike(18, 64)
    lin0, lin1, act2, key = me.find_mlp_encoder(vis, _obs((18, 18)))
    assert (lin0, lin1, act2, key) == (vis.fc1, vis.fc2, "tanh", "obs")
    for act in ("relu", "tanh", "none"):
        own = ssa.nets.MlpEncoder((6, 3), 32, 5, out_act=act, key="grid")
        assert me.find_mlp_encoder(own) == (own.fc1, own.fc2, act, "grid")
        assert own.embedding_dim == 5
    # cached on the encoder object: the second question is answered without the observations
    assert me.find_mlp_encoder(enc)[2] == "relu" and me.is_mlp_encoder(enc)


def test_a_linear_output_is_recognised_as_none():
    class Plain(_Base):
        def __init__(self):
            super().__init__(4)
            self.a, self.b = nn.Linear(8, 32), nn.Linear(32, 4)

        def forward(self, o):
            return self.b(F.relu(self.a(o["obs"])))
    assert me.find_mlp_encoder(Plain(), _obs((8,)))[2] == "none"


@pytest.mark.parametrize("cls", [ThreeLinears, TanhHidden, NormBetween])
def test_recognition_refuses_other_modules_with_todays_message(cls):
    enc = cls()
    assert me.find_mlp_encoder(enc, _obs()) is None
    with pytest.raises(NotImplementedError, match=REFUSAL):
        lu.encode(enc, _obs())


def test_recognition_refuses_two_candidate_keys():
    enc = mc.SharedEncoderLike(11, 64)
    obs = {"obs": torch.zeros(2, 11), "goal": torch.zeros(2, 11)}
    assert me.find_mlp_encoder(enc, obs) is None
    with pytest.raises(NotImplementedError, match=REFUSAL):
        lu.encode(enc, obs)


def test_identity_and_pixel_encoders_are_not_mlp_encoders():
    assert me.find_mlp_encoder(ssa.nets.IdentityEncoder(11), _obs()) is None
    pix = ssa.nets.PixelEncoder(ssa.nets.SmallPixelEncoder((3, 84, 84), 50))
    assert me.find_mlp_encoder(pix) is None


def test_the_probe_leaves_every_global_generator_alone():
    torch.manual_seed(5); np.random.seed(5); random.seed(5)
    shared, vis, other = mc.SharedEncoderLike(11, 64), mc.VisgridEncoderLike(18, 64), TanhHidden()   # (their init draws)
    t0, n0, p0 = torch.get_rng_state(), np.random.get_state(), random.getstate()
    assert me.find_mlp_encoder(shared, _obs()) is not None
    assert me.find_mlp_encoder(vis, _obs((18, 18))) is not None
    assert me.find_mlp_encoder(other, _obs()) is None
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n1[0] == n0[0] and np.array_equal(n1[1], n0[1]) and n1[2:] == n0[2:]
    assert random.getstate() == p0


def test_arena_layout_and_binding():
    offs, total = me.arena_layout([64 * 11, 64, 11 * 64, 11])
    assert all(o % 4 == 0 for o in offs) and total % 4 == 0 and offs == [0, 704, 768, 1472] and total == 1484
    offs, total = me.arena_layout([3, 5, 2, 1])
    assert offs == [0, 4, 12, 16] and total == 20
    enc = mc.SharedEncoderLike(11, 64)
    before = [p.detach().clone() for p in enc.parameters()]
    eng = me.MlpEncoderEngine(enc, me.find_mlp_encoder(enc, _obs()), "cpu")
    assert all(o % 4 == 0 for o in eng.offs) and eng.numel == 1484 and eng.grads.shape == eng.flat.shape
    assert eng.is_bound() and (eng.K, eng.H, eng.emb, eng.act2) == (11, 64, 11, 1)
    # the values moved with the parameters, the dummy Linear(1, 1) stays outside the arena
    assert all(torch.equal(a, b) for a, b in zip(before, enc.parameters()))
    assert all(p is not enc.have_at_least_one_param.weight and p is not enc.have_at_least_one_param.bias for p in eng.plist)
    with torch.no_grad():
        eng.flat.add_(1.0)
    assert torch.equal(enc.fc0.weight, before[2] + 1.0)   # (parameters(): dummy weight, dummy bias, fc0.weight, ...)
    # load_state_dict copies in place: still bound; a deepcopy clones the parameters: the copy's engine is not
    enc.load_state_dict({k: v.clone() for k, v in enc.state_dict().items()})
    assert eng.is_bound()
    enc.__dict__["_ssac_mlp"] = eng
    twin = copy.deepcopy(enc)
    assert not twin.__dict__["_ssac_mlp"].is_bound()
    assert eng.is_bound()
