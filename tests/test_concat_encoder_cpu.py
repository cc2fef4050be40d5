"""CPU: recognition of concatenating encoders (adopt.probe_concat, nets.ConcatEncoder) and what the recording gates make
of an agent that has one.  No GPU, no kernel.

An encoder that lays several vector keys side by side counts as an identity encoder over the wider row.  The probe runs
four random rows from a local generator through the encoder and asks for the keys' columns, bit for bit, in some order
that uses every key exactly once; everything else keeps the refusal of an encoder of no known kind."""
import random
import types

import numpy as np
import pytest
import torch
from torch import nn

import super_sac_amd as ssa
from super_sac_amd import adopt
from super_sac_amd import learning_utils as lu

WIDTHS = {"obs": 5, "goal": 2, "task": 4}


def _rows(widths=WIDTHS, n=1):
    g = torch.Generator().manual_seed(5)
    return {k: torch.randn(n, w, generator=g) for k, w in widths.items()}


class _Base(ssa.nets.Encoder):
    embedding_dim = 11


class UserGoalEncoder(_Base):
    """written as a user would: the reference's Encoder base, a torch.cat in forward"""
    embedding_dim = 7

    def forward(self, o):
        return torch.cat([o["goal"], o["obs"]], 1)


class Permuted(_Base):
    def forward(self, o):
        return torch.cat([o["task"], o["obs"], o["goal"]], dim=1)


class Unused(_Base):
    embedding_dim = 9

    def forward(self, o):
        return torch.cat([o["obs"], o["task"]], 1)


class Repeated(_Base):
    def forward(self, o):   # (the right width, but "goal" is never used and two columns of "obs" come twice)
        return torch.cat([o["obs"], o["obs"][:, :2], o["task"]], 1)


class Scaled(_Base):
    def forward(self, o):
        return 2.0 * torch.cat([o["obs"], o["goal"], o["task"]], 1)


class Shifted(_Base):
    def forward(self, o):
        return torch.cat([o["obs"], o["goal"], o["task"]], 1) + 1.0


class WithParameters(_Base):
    def __init__(self):
        super().__init__()
        self.gain = nn.Parameter(torch.ones(1))

    def forward(self, o):
        return torch.cat([o["obs"], o["goal"], o["task"]], 1) * self.gain


class WithBuffer(_Base):
    """a running normaliser keeps state in buffers: it is never fed probe rows"""

    def __init__(self):
        super().__init__()
        self.register_buffer("seen", torch.zeros(1))

    def forward(self, o):
        self.seen += 1
        return torch.cat([o["obs"], o["goal"], o["task"]], 1)


class SingleKeyCopy(_Base):
    embedding_dim = 5

    def forward(self, o):
        return o["obs"].clone()


class ReferenceIdentity(_Base):
    """the reference scripts' identity encoder (experiments/gym/train_gym.py:18-28)"""
    embedding_dim = 5

    def forward(self, o):
        return o["obs"]


class ImageKey(_Base):
    def forward(self, o):
        return torch.cat([o["obs"], o["img"].flatten(1)], 1)


def test_the_package_class():
    enc = ssa.nets.ConcatEncoder(WIDTHS)
    assert enc.embedding_dim == 11 and enc.ssac_concat_keys == (("obs", 5), ("goal", 2), ("task", 4))
    o = _rows(n=3)
    assert torch.equal(enc(o), torch.cat([o["obs"], o["goal"], o["task"]], 1))
    enc = ssa.nets.ConcatEncoder(WIDTHS, order=["task", "obs", "goal"])
    assert enc.ssac_concat_keys == (("task", 4), ("obs", 5), ("goal", 2))
    assert torch.equal(enc(o), torch.cat([o["task"], o["obs"], o["goal"]], 1))
    assert lu.is_identity(enc) and adopt.probe_concat(enc, None) == enc.ssac_concat_keys
    assert [n for n, _ in enc.named_parameters()] == ["have_at_least_one_param.weight", "have_at_least_one_param.bias"]
    with pytest.raises(AssertionError):
        ssa.nets.ConcatEncoder(WIDTHS, order=["obs", "goal"])


def test_a_users_encoder_is_recognised():
    enc = UserGoalEncoder()
    assert not lu.is_identity(enc)
    rows = _rows({"obs": 5, "goal": 2})
    assert adopt.probe_identity(enc, rows) is None
    assert adopt.probe_concat(enc, rows) == (("goal", 2), ("obs", 5))
    assert enc.ssac_concat_keys == (("goal", 2), ("obs", 5)) and lu.is_identity(enc)


def test_a_permuted_order_is_found_and_cached():
    enc = Permuted()
    assert adopt.probe_concat(enc, _rows()) == (("task", 4), ("obs", 5), ("goal", 2))
    calls = []
    enc.forward = lambda o: calls.append(1)   # the second ask does not run the encoder again
    assert adopt.probe_concat(enc, _rows()) == (("task", 4), ("obs", 5), ("goal", 2)) and not calls
    assert adopt.probe_concat(enc, None) == (("task", 4), ("obs", 5), ("goal", 2))
    # ... and neither does the second ask of an encoder that is none
    other = Scaled()
    assert adopt.probe_concat(other, _rows()) is None
    other.forward = lambda o: calls.append(1)
    assert adopt.probe_concat(other, _rows()) is None and not calls


def test_the_probe_moves_no_global_stream():
    yes, no, rows = Permuted(), Scaled(), _rows()   # (building a module initialises its Linear(1, 1) from torch's stream)
    random.seed(3), np.random.seed(3), torch.manual_seed(3)
    before = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2], torch.get_rng_state().clone())
    assert adopt.probe_concat(yes, rows) is not None
    assert adopt.probe_concat(no, rows) is None
    assert random.getstate() == before[0]
    assert np.array_equal(np.random.get_state()[1], before[1]) and np.random.get_state()[2] == before[2]
    assert torch.equal(torch.get_rng_state(), before[3])


def test_the_probe_keeps_the_training_flag():
    for flag in (True, False):
        enc = Permuted()
        enc.train(flag)
        adopt.probe_concat(enc, _rows())
        assert enc.training is flag


@pytest.mark.parametrize("cls", [Unused, Repeated, Scaled, Shifted, WithParameters, WithBuffer, ImageKey, SingleKeyCopy])
def test_everything_else_keeps_todays_refusal(cls):
    enc = cls()
    rows = _rows()
    if cls is ImageKey:
        rows = {"obs": rows["obs"], "img": torch.zeros(1, 1, 2, 3)}
    if cls is SingleKeyCopy:
        rows = {"obs": rows["obs"]}
    assert adopt.probe_identity(enc, rows) is None
    assert adopt.probe_concat(enc, rows) is None
    assert not lu.is_identity(enc) and getattr(enc, "ssac_concat_keys", None) is None
    with pytest.raises(NotImplementedError) as err:
        lu.encode(enc, rows)
    assert str(err.value) == f"{cls.__name__}: this encoder has no HIP path"
    if cls is WithBuffer:
        assert float(enc.seen) == 1.0   # (probe_identity's one buffer row, as before; no probe rows)


@pytest.mark.parametrize("first", ["acting", "update"])
def test_a_single_key_identity_encoder_stays_an_identity_encoder(first):
    """the reference's identity encoder hands its one key back: whichever call meets it first -- an acting call (the
    reference loop acts before it updates) or an update -- it ends as an identity encoder, never as a one-key
    concatenation, and the buffer gets no column order (its gather stays foldable into the chained launch)"""
    from super_sac_amd import acting
    enc = ReferenceIdentity()
    actor = types.SimpleNamespace(dist_impl=None)
    agent = types.SimpleNamespace(encoder=enc, actors=[actor], critics=[types.SimpleNamespace()], act_space_size=2,
                                  ucb_bonus=0.0, discrete=False, _ssac_adopted=True)
    storage = types.SimpleNamespace(s_stack={"obs": torch.zeros(6, 5)})
    buffer = types.SimpleNamespace(_storage=storage, draw_uniform_indices=None)
    obs = {"obs": np.zeros(5, np.float32)}
    if first == "acting":
        assert acting._eligible(agent, obs, 1, True, False) is False   # (nobody has recognised it yet: the general path)
        assert getattr(enc, "ssac_concat_keys", None) is None and "_ssac_concat_probed" not in enc.__dict__
    lu.ensure_adopted(agent, buffer)
    assert enc.ssac_identity_key == "obs" and getattr(enc, "ssac_concat_keys", None) is None
    assert lu.concat_order(storage) is None
    assert acting._eligible(agent, obs, 1, False, False) is True
    # ... and the probe itself refuses a single key
    assert adopt.probe_concat(ReferenceIdentity(), {"obs": torch.zeros(1, 5)}) is None


def test_ensure_adopted_finds_it_and_sets_the_buffers_order():
    enc = Permuted()
    storage = types.SimpleNamespace(s_stack={k: torch.zeros(6, w) for k, w in WIDTHS.items()})
    buffer = types.SimpleNamespace(_storage=storage, draw_uniform_indices=None)
    agent = types.SimpleNamespace(encoder=enc, _ssac_adopted=True)
    lu.ensure_adopted(agent, buffer)
    want = (("task", 4), ("obs", 5), ("goal", 2))
    assert enc.ssac_concat_keys == want and lu.concat_order(storage) == want
    lu.ensure_adopted(agent, buffer)   # (again: nothing to do)
    # a second agent with the same order shares the buffer, one with another order is refused with a reason
    lu.ensure_adopted(types.SimpleNamespace(encoder=ssa.nets.ConcatEncoder(WIDTHS, ["task", "obs", "goal"]),
                                            _ssac_adopted=True), buffer)
    with pytest.raises(NotImplementedError, match="already laid out as .'task', 'obs', 'goal'. for another agent"):
        lu.ensure_adopted(types.SimpleNamespace(encoder=ssa.nets.ConcatEncoder(WIDTHS), _ssac_adopted=True), buffer)
    assert lu.concat_order(storage) == want
    # an encoder whose keys are not the buffer's
    other = types.SimpleNamespace(_storage=types.SimpleNamespace(s_stack={"obs": torch.zeros(6, 5)}), draw_uniform_indices=None)
    with pytest.raises(NotImplementedError, match="every key of the buffer must be a vector the encoder uses exactly once"):
        lu.ensure_adopted(types.SimpleNamespace(encoder=ssa.nets.ConcatEncoder(WIDTHS), _ssac_adopted=True), other)
    assert lu.concat_order(other._storage) is None


def _call(encoder, E=1, widths=None):
    critics = [types.SimpleNamespace() for _ in range(E)]
    actors = [types.SimpleNamespace(dist_impl=None) for _ in range(E)]
    agent = types.SimpleNamespace(actors=actors, critics=critics, ensemble_size=E, popart=[False] * E, encoder=encoder)
    storage = types.SimpleNamespace(s_stack={k: torch.zeros(3, w) for k, w in (widths or {"obs": 5, "goal": 2}).items()})
    buffer = types.SimpleNamespace(_storage=storage, per_on_device=True)
    return dict(agent=agent, buffer=buffer, discrete=False, random_process=None, per=False, update_priorities=False,
                dr3_coeff=0.0, weight_type=None, weighted_bellman_temp=None, log_alphas=[torch.zeros(1)])


def test_the_gates_see_an_identity_encoder_over_a_dictionary_buffer():
    enc = UserGoalEncoder()
    assert adopt.probe_concat(enc, _rows({"obs": 5, "goal": 2})) is not None
    f = lu.call_facts(_call(enc), "list", True, True)
    assert f.identity_encoder is True and f.vector_obs is False and f.ensemble_size == 1
    # (cuda is a fact of the machine; the verdict is asked as on the GPU box)
    v = lu.recording_verdict(f._replace(cuda=True))
    assert v.record is True and v.members is False
    # more than one member: the members form needs vector_obs, so the call stays eager
    f2 = lu.call_facts(_call(enc, E=2), "list", True, True)
    v2 = lu.recording_verdict(f2._replace(cuda=True))
    assert f2.identity_encoder and not f2.vector_obs and v2.members is False and v2.record is False
    # an encoder of no known kind over the same buffer: not an identity, nothing is recorded
    f3 = lu.call_facts(_call(Scaled()), "list", True, True)
    assert f3.identity_encoder is False and lu.recording_verdict(f3._replace(cuda=True)).record is False
