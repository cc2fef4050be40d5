"""CPU: what the trainable-encoder engines share (super_sac_amd/encoder_base.py) -- the arena packing, the one cache rule of
the lookup, the accumulate form of backward and the refusal.  Engines are built on "cpu"; nothing is launched."""
import copy

import pytest
import torch
from torch import nn

import mlp_encoder_cases as mc
import super_sac_amd as ssa
from super_sac_amd import conv_encoder as ce
from super_sac_amd import encoder_base as eb
from super_sac_amd import mlp_encoder as me

OBS = {"obs": torch.zeros(3, 11)}
KINDS = {
    "pixel": (lambda: ssa.nets.PixelEncoder(ssa.nets.SmallPixelEncoder((4, 36, 36))), None, ce.ConvEncoderEngine),
    "conv_stack": (lambda: ssa.nets.ConvStackEncoder((4, 10, 10)), None, ce.ConvEncoderEngine),
    "mlp": (lambda: ssa.nets.MlpEncoder(11, 64, 11), None, me.MlpEncoderEngine),
    "adopted": (lambda: mc.SharedEncoderLike(11, 64), OBS, me.MlpEncoderEngine),
}
EACH = pytest.mark.parametrize("kind", list(KINDS))


@EACH
def test_packing(kind):
    make, obs, cls = KINDS[kind]
    torch.manual_seed(0)
    enc = make()
    with torch.no_grad():
        for p in enc.parameters():   # (biases start at zero: give every element a value of its own)
            p.add_(torch.randn(p.shape))
    before = [p.detach().clone() for p in enc.parameters()]
    eng = eb.encoder_engine(enc, "cpu", obs)
    assert isinstance(eng, eb.EncoderEngine) and type(eng) is cls
    assert eng.moments_key == {ce.ConvEncoderEngine: "conv_encoder", me.MlpEncoderEngine: "mlp_encoder"}[cls]
    offs, total = eb.arena_layout([p.numel() for p in eng.plist])
    assert eng.offs == offs and eng.numel == total == eng.flat.numel() and all(o % 4 == 0 for o in eng.offs)
    assert eng.grads.shape == eng.flat.shape and eng.grads.data_ptr() != eng.flat.data_ptr()
    assert eng.is_bound()
    assert all(torch.equal(a, b) for a, b in zip(before, enc.parameters())), "packing changed a parameter"
    for k, p in enumerate(eng.plist):
        assert torch.equal(eng._seg(k), p.detach().reshape(-1)) and eng._seg(k, eng.grads).numel() == p.numel()
    held = {id(p) for p in eng.plist}
    moved = [(p, b) for p, b in zip(enc.parameters(), before) if id(p) in held]
    assert len(moved) == len(eng.plist)
    with torch.no_grad():
        eng.flat.add_(1)
    assert all(torch.equal(p, b + 1) for p, b in moved), "the parameters do not live in the arena"


@EACH
def test_one_cache_rule(kind):
    make, obs, _ = KINDS[kind]
    enc = make()
    eng = eb.encoder_engine(enc, "cpu", obs)
    assert eb.encoder_engine(enc, torch.device("cpu"), obs) is eng and eb.require_engine(enc, "cpu", obs) is eng
    per_kind = ce.conv_engine(enc, "cpu") if isinstance(eng, ce.ConvEncoderEngine) else me.mlp_engine(enc, "cpu", obs)
    assert per_kind is eng
    twin = copy.deepcopy(enc)   # (clones every parameter: the copied cache slot holds an engine they left)
    teng = eb.encoder_engine(twin, "cpu", obs)
    assert teng is not eng and teng.module is not eng.module and teng.is_bound()
    assert teng.flat.data_ptr() != eng.flat.data_ptr()
    assert eb.encoder_engine(twin, "cpu", obs) is teng
    assert eng.is_bound() and eb.encoder_engine(enc, "cpu", obs) is eng
    # parameters that left the arena by any other road: re-packed as well
    with torch.no_grad():
        teng.plist[0].data = teng.plist[0].data.clone()
    assert not teng.is_bound()
    again = eb.encoder_engine(twin, "cpu", obs)
    assert again is not teng and again.is_bound()


class _Stub(eb.EncoderEngine):
    moments_key = "stub"

    def __init__(self):
        self.module = None
        self._pack([nn.Parameter(torch.zeros(5)), nn.Parameter(torch.zeros(2, 3))], "cpu")
        self.seen = []

    def _backward(self, d_rep):
        self.seen.append(self.grads)
        self.grads.copy_(torch.arange(1.0, self.numel + 1.0) * d_rep)


def test_accumulate_wrapper():
    eng = _Stub()
    assert eng.offs == [0, 8] and eng.numel == 16
    grads, pattern = eng.grads, torch.arange(1.0, 17.0) * 3.0
    eng.backward(3.0)
    assert eng.grads is grads and torch.equal(grads, pattern)
    eng.backward(3.0, accumulate=True)
    assert eng.grads is grads and torch.equal(grads, 2 * pattern)
    assert eng.seen[0] is grads and eng.seen[1] is not grads, "the accumulating pass must fill a buffer of its own"
    eng.backward(3.0)
    assert eng.grads is grads and torch.equal(grads, pattern)

    class Failing(_Stub):
        def _backward(self, d_rep):
            raise RuntimeError("launch failed")
    bad = Failing()
    keep = bad.grads
    with pytest.raises(RuntimeError, match="launch failed"):
        bad.backward(1.0, accumulate=True)
    assert bad.grads is keep


class _ThreeLinears(nn.Module):
    embedding_dim = 11

    def __init__(self):
        super().__init__()
        self.a, self.b, self.c = nn.Linear(11, 32), nn.Linear(32, 32), nn.Linear(32, 11)

    def forward(self, o):
        return self.c(self.b(self.a(o["obs"])))


def test_refusal():
    enc = _ThreeLinears()
    assert eb.encoder_engine(enc, "cpu", OBS) is None
    with pytest.raises(NotImplementedError, match="_ThreeLinears: this encoder has no HIP path"):
        eb.require_engine(enc, "cpu", OBS)
    assert eb.encoder_engine(ssa.nets.IdentityEncoder(11), "cpu", OBS) is None
