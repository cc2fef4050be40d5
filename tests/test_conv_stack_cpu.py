"""CPU: recognition of plain conv-stack encoders (super_sac_amd/conv_encoder.py), the coverage predicate of the fused
kernels at its edges, and the fp32-vs-fp64 measurement the GPU tests take their bounds from."""
import copy
import random

import numpy as np
import pytest
import torch
from torch import nn

import conv_stack_cases as cc
import super_sac_amd as ssa
from super_sac_amd import conv_encoder as ce
from super_sac_amd._lib import lib

REFUSAL = "this encoder has no HIP path"
MINATAR = (16, 3, 1, 16, 2, 1)   # co1, k1, s1, co2, k2, s2


@pytest.mark.parametrize("div", [1.0, 255.0])
@pytest.mark.parametrize("channels", [1, 4, 10])
def test_probe_finds_the_input_normalisation(div, channels):
    enc = cc.MinAtarLike(channels, div=div)
    assert "ssac_obs_key" not in enc.__dict__
    assert ce.find_conv_module(enc) is enc
    assert ce.conv_input(enc) == (div, 0.0)
    assert enc.__dict__["ssac_obs_key"] == "obs" and enc.__dict__["_ssac_conv_input"] == (div, 0.0)
    # a deepcopy (the target network) carries the result and is not probed again
    twin = copy.deepcopy(enc)
    assert ce.find_conv_module(twin) is twin and ce.conv_input(twin) == (div, 0.0)


def test_probe_needs_no_frame_shape():
    """a stack on 9 x 8 frames (last map 6 x 5): probed on some frame whose last map has 30 pixels"""
    enc = cc.MinAtarLike(3, (9, 8), 7, 255.0, ((16, 2, 1), (16, 3, 1)))
    assert ce.find_conv_module(enc) is enc and ce.conv_input(enc) == (255.0, 0.0)


def test_probe_result_is_cached(monkeypatch):
    enc = cc.MinAtarLike(4)
    ce.find_conv_module(enc)
    monkeypatch.setattr(ce, "_probe_stack", lambda *a: pytest.fail("probed twice"))
    assert ce.find_conv_module(enc) is enc


@pytest.mark.parametrize("cls", [cc.SigmoidStackLike, cc.NhwcFlattenLike])
def test_probe_refuses_what_matches_no_candidate(cls, monkeypatch):
    enc = cls(4)
    with pytest.raises(NotImplementedError, match=f"{cls.__name__}: {REFUSAL}"):
        ce.find_conv_module(enc)
    with pytest.raises(NotImplementedError, match=REFUSAL):
        ce.conv_engine(enc, "cpu")
    # ... also where the module used to be waved through as "a pixel encoder", and the refusal is remembered
    monkeypatch.setattr(ce, "_probe_stack", lambda *a: pytest.fail("probed twice"))
    with pytest.raises(NotImplementedError, match=REFUSAL):
        ssa.adopt.probe_identity(enc, {"obs": torch.zeros(1, 4, 10, 10)})


def test_structure_outside_a_plain_stack_is_refused():
    padded = cc.MinAtarLike(4)
    padded.conv1 = nn.Conv2d(4, 16, 3, padding=1)
    padded.fc = nn.Linear(16 * 9 * 9, 50)
    with pytest.raises(NotImplementedError, match=REFUSAL):
        ce.find_conv_module(padded)
    gap = cc.MinAtarLike(4)
    gap.conv3 = gap.conv2
    del gap.conv2
    with pytest.raises(NotImplementedError, match=REFUSAL):
        ce.find_conv_module(gap)


def test_probe_leaves_the_global_generators_alone():
    good, odd = cc.MinAtarLike(7, div=255.0), cc.SigmoidStackLike(7)   # (building them draws their initial weights)
    torch.manual_seed(11); np.random.seed(12); random.seed(13)
    before = (torch.get_rng_state().clone(), np.random.get_state()[1].copy(), random.getstate())
    ce.find_conv_module(good)
    with pytest.raises(NotImplementedError):
        ce.find_conv_module(odd)
    assert torch.equal(torch.get_rng_state(), before[0])
    assert np.array_equal(np.random.get_state()[1], before[1]) and random.getstate() == before[2]


def test_known_pixel_encoders_are_not_probed(monkeypatch):
    monkeypatch.setattr(ce, "_probe_stack", lambda *a: pytest.fail("a known pixel encoder was probed"))
    small, big = ssa.nets.SmallPixelEncoder((4, 84, 84)), ssa.nets.BigPixelEncoder((9, 64, 64))
    for block, want in ((small, (255.0, 0.0)), (big, (255.0, -0.5))):
        enc = ssa.nets.PixelEncoder(block)
        assert ce.find_conv_module(enc) is block and ce.conv_input(block) == want
        assert "_ssac_conv_input" not in block.__dict__

    class SmallPixelEncoder(nn.Module):   # a reference-built module is known by its class name
        def __init__(self):
            super().__init__()
            self.conv1, self.fc = nn.Conv2d(4, 32, 8, 4), nn.Linear(32, 50)

    class WithLn(nn.Module):              # ... and anything with `ln` keeps today's path
        def __init__(self):
            super().__init__()
            self.conv1, self.fc, self.ln = nn.Conv2d(4, 32, 3), nn.Linear(32, 50), nn.LayerNorm(50)
    for block, want in ((SmallPixelEncoder(), (255.0, 0.0)), (WithLn(), (255.0, -0.5))):
        assert ce.find_conv_module(block) is block and ce.conv_input(block) == want


def test_conv_stack_encoder_declares_its_function(monkeypatch):
    monkeypatch.setattr(ce, "_probe_stack", lambda *a: pytest.fail("nets.ConvStackEncoder was probed"))
    enc = ssa.nets.ConvStackEncoder((4, 10, 10))
    assert isinstance(enc, ssa.nets.Encoder) and enc.embedding_dim == 50 and enc.ssac_obs_key == "obs"
    assert (enc.conv1.in_channels, enc.conv1.out_channels, enc.conv1.kernel_size) == (4, 16, (3, 3))
    assert (enc.conv2.in_channels, enc.conv2.out_channels, enc.conv2.kernel_size) == (16, 16, (2, 2))
    assert (enc.fc.in_features, enc.fc.out_features) == (784, 50)
    assert ce.find_conv_module(enc) is enc and ce.conv_input(enc) == (1.0, 0.0)
    other = ssa.nets.ConvStackEncoder((3, 9, 8), convs=((16, 2, 1), (16, 3, 1)), out_dim=7, input_div=255.0, key="pixels")
    assert ce.conv_input(other) == (255.0, 0.0) and other.fc.in_features == 16 * 6 * 5 and other.ssac_obs_key == "pixels"
    # it computes stack_function of its own tensors (checked against the stand-in holding the same weights)
    twin = cc.MinAtarLike(4)
    cc.load_encoder(twin, {"p": cc.encoder_tensors(enc)})
    x = torch.randint(0, 2, (3, 4, 10, 10), generator=torch.Generator().manual_seed(1)).float()
    with torch.no_grad():
        assert torch.equal(twin({"obs": x}), ce.stack_function(x, [enc.conv1, enc.conv2], enc.fc, 1.0, 0.0))


def test_covered_at_its_edges():
    cov = lambda C, H, W, geo=MINATAR: bool(lib.ssac_enc_convstack_covered(C, H, W, *geo))
    assert all(cov(C, 10, 10) for C in range(1, 17))
    assert not cov(0, 10, 10) and not cov(17, 10, 10)
    # 16 output channels, stride 1, kernels up to 4
    for geo in ((32, 3, 1, 16, 2, 1), (16, 3, 1, 8, 2, 1), (16, 3, 2, 16, 2, 1), (16, 3, 1, 16, 2, 2), (16, 5, 1, 16, 2, 1),
                (16, 3, 1, 16, 5, 1), (16, 0, 1, 16, 2, 1)):
        assert not cov(4, 10, 10, geo), geo
    assert cov(4, 10, 10, (16, 4, 1, 16, 4, 1)) and cov(3, 9, 8, (16, 2, 1, 16, 3, 1))
    # the frame holds both kernels, sides up to 32
    assert cov(4, 4, 4) and not cov(4, 3, 4) and not cov(4, 4, 3)
    assert cov(1, 4, 32) and not cov(1, 4, 33) and not cov(1, 33, 4)
    # a tile's working set within 64 KiB of LDS: 12 x 12 frames fit with 4 channels, not with 16; 16 x 16 frames do not fit
    assert cov(4, 12, 12) and not cov(16, 12, 12) and not cov(1, 16, 16)


def test_supported_implies_covered_and_follows_the_measurement():
    """profiles/conv_stack_encoder.md: the default takes the fused form only where it measured faster"""
    sup = lambda B, C, H=10, W=10, geo=MINATAR: bool(lib.ssac_enc_convstack_supported(B, C, H, W, *geo))
    assert not sup(32, 17) and not sup(0, 4) and not sup(32, 4, 16, 16)
    # measured: MinAtar's geometry between the corners C 1 .. 16, B 1 .. 1024
    assert all(sup(B, C) for B in (1, 8, 32, 256, 1024) for C in (1, 4, 10, 16))
    assert not sup(1025, 4)
    # not measured, so not the default, though covered
    assert not sup(32, 4, 12, 12) and not sup(32, 3, 9, 8, (16, 2, 1, 16, 3, 1)) and not sup(32, 4, 10, 10, (16, 2, 1, 16, 2, 1))
    assert ce.STACK_FUSED is True


def test_exact_inputs_are_exact_and_the_bounds_are_measured():
    """(a) on the 2^-6 grid torch's fp32 CPU result IS the fp64 result, so the GPU tests may ask for bit equality; (b) on
    Gaussian inputs the fp32-vs-fp64 distance gives a bound above the ulp floor and far below the values' size"""
    x, p, d_flat = cc.grid_case(5, 14, 7)
    r32, r64 = cc.reference(x, p, 1.0, torch.float32, d_flat=d_flat), cc.reference(x, p, 1.0, torch.float64, d_flat=d_flat)
    for k in ("h1", "flat", "gw1", "gb1", "gw2", "gb2"):
        assert torch.equal(r32[k].double(), r64[k]), k
        assert float(r64[k].abs().max()) > 0
    x, p, d_flat, d_emb = cc.gauss_case(6, 14, 7)
    r32, r64 = cc.reference(x, p, 255.0, torch.float32, d_emb=d_emb), cc.reference(x, p, 255.0, torch.float64, d_emb=d_emb)
    for k in ("h1", "flat", "emb", "gw1", "gb1", "gw2", "gb2", "gwf", "gbf"):
        bound, size = cc.measured_bound(r32[k], r64[k]), float(r64[k].abs().max())
        assert np.spacing(np.float32(size)) <= bound <= 1e-4 * size, (k, bound, size)
