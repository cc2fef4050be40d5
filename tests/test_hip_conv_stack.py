"""GPU: the conv-stack launches (csrc/ssac_enc_convstack.hip) through the C ABI and the engine's gradients in both launch
forms (conv_encoder.STACK_FUSED "all" / False), per element against fp64.

Inputs (conv_stack_cases): (a) 0/1 pixels with weights and d(flat) on a 2^-6 grid -- every fp32 sum is exact, so h1, the
flatten and every gradient are compared BIT FOR BIT with the float64 reference; (b) Gaussian weights, uint8 pixels 0..255
under div = 255 -- the bound per quantity is 4 x the largest |torch fp32 CPU - fp64| on the same inputs, never below one fp32
ulp of the largest magnitude (measured_bound, the rule of tests/test_hip_mlp_encoder.py); the worst ratio per quantity is
printed for profiles/conv_stack_encoder.md.

Measured on an MI355X (worst |result - fp64| / bound over all cases): fused launches h1 0.37, flatten 0.37, dW1 0.39, db1 0.69,
dW2 0.45, db2 0.78; engine gradients at most 0.54 of their bound in the fused form and 0.97 (db2) per layer.
"""
import numpy as np
import pytest
import torch

import conv_stack_cases as cc

pytestmark = pytest.mark.gpu

R = 4   # SSAC_ENC_CONVSTACK_TILE
# (channels, (H, W), convs): MinAtar's geometry at every channel count class, and one other covered geometry (non-square
# frame, the larger kernel second, pixel counts 56 and 30: ragged 16-pixel tiles in both layers)
GEOMETRIES = [(c, (10, 10), cc.CONVS) for c in (1, 4, 7, 10, 16)] + [(3, (9, 8), ((16, 2, 1), (16, 3, 1)))]
GEO_IDS = [f"C{c}-{h}x{w}-k{v[0][1]}k{v[1][1]}" for c, (h, w), v in GEOMETRIES]
BATCHES = [1, 2, R - 1, R, R + 1, 3 * R + 2]
SENTINEL = 24   # NaN words kept behind every output
_CACHE = {}


def _refs(kind, geo, B):
    """inputs and references of one case, computed once and shared (never modified)"""
    key = (kind, GEO_IDS[GEOMETRIES.index(geo)], B)
    if key not in _CACHE:
        c, hw, convs = geo
        seed = 100 + 31 * c + B
        if kind == "grid":
            x, p, d_flat = cc.grid_case(seed, B, c, hw, convs)
            ref = cc.reference(x, p, 1.0, torch.float64, d_flat=d_flat)
            _CACHE[key] = (x, p, d_flat, 1.0, ref, None)
        else:
            x, p, d_flat, _ = cc.gauss_case(seed, B, c, hw, 50, convs)
            conv_p = {k: p[k] for k in ("w1", "b1", "w2", "b2")}
            ref = cc.reference(x, conv_p, 255.0, torch.float64, d_flat=d_flat)
            r32 = cc.reference(x, conv_p, 255.0, torch.float32, d_flat=d_flat)
            _CACHE[key] = (x, conv_p, d_flat, 255.0, ref, {k: cc.measured_bound(r32[k], ref[k]) for k in ref})
    return _CACHE[key]


def _padded(n):
    return torch.full((n + SENTINEL,), float("nan"), device="cuda")


def _geo_args(geo):
    c, (h, w), ((co1, k1, s1), (co2, k2, s2)) = geo
    return c, h, w, co1, k1, s1, co2, k2, s2


def _run_fused(x, p, d_flat, div, geo, B):
    """fwd + bwd + the fixed-order reduction through the C ABI; every output with NaN sentinel words behind it"""
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    c, (h, w), convs = geo
    args = _geo_args(geo)
    assert lib.ssac_enc_convstack_covered(*args) == 1
    st = engine.stream()
    d = {k: v.cuda().contiguous() for k, v in p.items()}
    (h1h, h1w), (h2h, h2w) = cc.out_hw(h, w, convs[:1]), cc.out_hw(h, w, convs)
    n1, n2 = 16 * h1h * h1w, 16 * h2h * h2w
    H1, flat = _padded(B * n1), _padded(B * n2)
    xd = x.cuda().contiguous()
    w_ptrs = (d["w1"].data_ptr(), d["b1"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr())
    check(lib.ssac_enc_convstack_fwd(xd.data_ptr(), 1, *w_ptrs, B, *args, div, 0.0, H1.data_ptr(), flat.data_ptr(), st))
    assert bool(torch.isnan(H1[B * n1:]).all()) and bool(torch.isnan(flat[B * n2:]).all()), "wrote behind an output"
    # float32 frames, and no H1: the same flatten, bit for bit
    xf = x.float().cuda().contiguous()
    flat2 = _padded(B * n2)
    check(lib.ssac_enc_convstack_fwd(xf.data_ptr(), 0, *w_ptrs, B, *args, div, 0.0, 0, flat2.data_ptr(), st))
    assert torch.equal(flat2[:B * n2], flat[:B * n2]) and bool(torch.isnan(flat2[B * n2:]).all())
    # backward: one partial per image tile, then ssac_reduce_slices
    n = 16 * (c * convs[0][1] ** 2 + 1) + 16 * (16 * convs[1][1] ** 2 + 1)
    slices = (B + R - 1) // R
    dfl = d_flat.cuda().contiguous()
    parts = []
    for frames, u8 in ((xd, 1), (xf, 0), (xd, 1)):
        part = _padded(slices * n)
        check(lib.ssac_enc_convstack_bwd(dfl.data_ptr(), frames.data_ptr(), u8, H1.data_ptr(), flat.data_ptr(),
                                         d["w2"].data_ptr(), B, *args, div, 0.0, part.data_ptr(), st))
        assert bool(torch.isnan(part[slices * n:]).all()), "wrote behind the partials"
        assert not bool(torch.isnan(part[:slices * n]).any()), "a partial element was left unwritten"
        parts.append(part)
    assert torch.equal(parts[0][:slices * n], parts[2][:slices * n]), "two runs of the backward differ"
    assert torch.equal(parts[0][:slices * n], parts[1][:slices * n]), "uint8 and float32 frames differ"
    grads = _padded(n)
    check(lib.ssac_reduce_slices(parts[0].data_ptr(), slices, n, grads.data_ptr(), st))
    assert bool(torch.isnan(grads[n:]).all())
    o1 = 16 * c * convs[0][1] ** 2
    o2 = o1 + 16
    o3 = o2 + 16 * 16 * convs[1][1] ** 2
    return {"h1": H1[:B * n1].view(B, n1), "flat": flat[:B * n2].view(B, n2), "gw1": grads[:o1].view(p["w1"].shape),
            "gb1": grads[o1:o2], "gw2": grads[o2:o3].view(p["w2"].shape), "gb2": grads[o3:n]}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
def test_fused_kernels_exact_on_the_grid(geo, B):
    x, p, d_flat, div, ref, _ = _refs("grid", geo, B)
    got = _run_fused(x, p, d_flat, div, geo, B)
    for k, v in got.items():
        assert float(ref[k].abs().max()) > 0
        assert torch.equal(v.double().cpu(), ref[k]), f"{k}: not the fp64 result bit for bit"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
def test_fused_kernels_within_the_measured_bound(geo, B):
    x, p, d_flat, div, ref, bounds = _refs("gauss", geo, B)
    got = _run_fused(x, p, d_flat, div, geo, B)
    for k, v in got.items():
        err = float((v.double().cpu() - ref[k]).abs().max())
        print(f"fused {k}: worst |kernel - fp64| {err:.3e}, bound {bounds[k]:.3e}, ratio {err / bounds[k]:.2f}")
        assert err <= bounds[k], f"{k}: {err:.3e} > {bounds[k]:.3e}"


def test_call_outside_the_covered_geometries_launches_nothing():
    from super_sac_amd import engine
    from super_sac_amd._lib import lib
    st = engine.stream()
    x = torch.zeros(2, 17, 10, 10, device="cuda")
    w1, b1, w2, b2 = (torch.zeros(n, device="cuda") for n in (16 * 17 * 9, 16, 1024, 16))
    out, h1, part = _padded(2 * 784), _padded(2 * 1024), _padded(16 * (17 * 9 + 64 + 2))
    for args in ((17, 10, 10, 16, 3, 1, 16, 2, 1), (4, 10, 10, 16, 3, 2, 16, 2, 1), (4, 10, 10, 32, 3, 1, 16, 2, 1),
                 (4, 16, 16, 16, 3, 1, 16, 2, 1)):
        assert lib.ssac_enc_convstack_covered(*args) == 0
        assert lib.ssac_enc_convstack_fwd(x.data_ptr(), 0, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 2,
                                          *args, 1.0, 0.0, h1.data_ptr(), out.data_ptr(), st) != 0
        assert lib.ssac_enc_convstack_bwd(out.data_ptr(), x.data_ptr(), 0, h1.data_ptr(), out.data_ptr(), w2.data_ptr(), 2,
                                          *args, 1.0, 0.0, part.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (out, h1, part)), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------------------------------
# the engine (conv layers AND fc, uint8 frames, x / 255) in both launch forms
# ---------------------------------------------------------------------------------------------------------------------
def _engine_refs(geo, B):
    key = ("engine", GEO_IDS[GEOMETRIES.index(geo)], B)
    if key not in _CACHE:
        c, hw, convs = geo
        x, p, _, d_emb = cc.gauss_case(700 + 31 * c + B, B, c, hw, 50, convs)
        ref, r32 = (cc.reference(x, p, 255.0, dt, d_emb=d_emb) for dt in (torch.float64, torch.float32))
        _CACHE[key] = (x, p, d_emb, ref, {k: cc.measured_bound(r32[k], ref[k]) for k in ref})
    return _CACHE[key]


def test_default_takes_the_fused_form_where_it_measured_faster():
    """profiles/conv_stack_encoder.md: MinAtar's geometry; the other covered geometry stays per layer, and so does every
    SmallPixelEncoder"""
    import super_sac_amd as ssa
    from super_sac_amd import conv_encoder as ce
    assert ce.STACK_FUSED is True
    dev = torch.device("cuda", torch.cuda.current_device())
    minatar = ce.conv_engine(ssa.nets.ConvStackEncoder((4, 10, 10)).cuda(), dev)
    other = ce.conv_engine(ssa.nets.ConvStackEncoder((3, 9, 8), convs=((16, 2, 1), (16, 3, 1))).cuda(), dev)
    small = ce.conv_engine(ssa.nets.PixelEncoder(ssa.nets.SmallPixelEncoder((4, 36, 36))).cuda(), dev)
    assert minatar.stack_fused(32, 10, 10) and minatar.stack_fused(1, 10, 10) and minatar.stack_fused(32, 10, 10, save=True)
    assert not minatar.stack_fused(31, 10, 10, save=True)   # (the fused backward lost at B 1; B 2 .. 31 is not measured)
    assert not other.stack_fused(32, 9, 8) and not small.stack_fused(32, 36, 36)
    for B, fused in ((32, True), (5, False)):
        emb = torch.empty(B, 50, device="cuda")
        minatar.forward(torch.zeros(B, 4, 10, 10, dtype=torch.uint8, device="cuda"), emb, 50, save=True)
        assert minatar.saved["fused"] == fused


@pytest.mark.parametrize("form", ["all", False], ids=["fused", "layers"])
@pytest.mark.parametrize("B", [1, R + 1, 3 * R + 2])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=GEO_IDS)
def test_engine_forward_and_gradients(geo, B, form):
    from super_sac_amd import conv_encoder as ce
    c, hw, convs = geo
    x, p, d_emb, ref, bounds = _engine_refs(geo, B)
    enc = cc.load_encoder(cc.MinAtarLike(c, hw, 50, 255.0, convs), {"p": p}).cuda()
    saved = ce.STACK_FUSED
    ce.STACK_FUSED = form
    try:
        eng = ce.conv_engine(enc, torch.device("cuda", torch.cuda.current_device()))
        assert (eng.div, eng.shift) == (255.0, 0.0) and eng.is_bound()
        assert eng.stack_fused(B, *hw, save=True) == (form == "all")
        xd = x.cuda()
        emb = torch.full((B, 53), float("nan"), device="cuda")
        eng.forward(xd, emb, 53, save=True)
        eng.backward(d_emb.cuda().contiguous())
        got = {"emb": emb[:, :50]}
        for i, (k, t) in enumerate(cc.encoder_tensors(enc).items()):   # (the arena's order: conv1, conv2, fc)
            assert eng.plist[i] is t
            got["g" + k] = eng._seg(i, eng.grads).view(t.shape)
        assert bool(torch.isnan(emb[:, 50:]).all()), "columns beyond the embedding were written"
        # the acting path (no save, float32 frames): the same embedding
        emb2 = torch.empty(B, 50, device="cuda")
        eng.forward(xd.float(), emb2, 50, save=False)
        assert torch.equal(emb2, emb[:, :50])
    finally:
        ce.STACK_FUSED = saved
    for k, v in got.items():
        err = float((v.double().cpu() - ref[k]).abs().max())
        print(f"engine {'fused' if form else 'layers'} {k}: worst |engine - fp64| {err:.3e}, bound {bounds[k]:.3e}, "
              f"ratio {err / bounds[k]:.2f}")
        assert err <= bounds[k], f"{k}: {err:.3e} > {bounds[k]:.3e}"
