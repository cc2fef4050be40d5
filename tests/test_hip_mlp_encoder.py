"""GPU: the MLP-encoder launches (csrc/ssac_enc_mlp.hip) and the engine's gradients, per element against fp64.

The tolerance is measured per shape (mlp_encoder_cases.measured_bound): 4 x the largest distance between torch's own fp32
CPU result and the fp64 result on the same inputs, never below one fp32 ulp of the largest magnitude involved.

Measured on an MI355X (worst |kernel - fp64| / the bound, at the shape where the ratio is largest): fused Y 1.98e-07 / 2.16e-07,
H_save 2.28e-06 / 5.51e-06, dZ1 1.06e-06 / 1.97e-06, dZ0 1.93e-07 / 3.11e-07; engine gradients at most 0.72 of their bound in
either form (profiles/mlp_encoder.md has the table).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_encoder_cases as mc

pytestmark = pytest.mark.gpu

ACT = {"none": 0, "relu": 1, "tanh": 2}
SHAPES = [(1, 11, 128, 11, "relu"),      # an acting row
          (5, 3, 128, 3, "relu"),        # Pendulum: K below one MFMA step
          (37, 17, 128, 17, "relu"),     # row tail, K and N tails
          (33, 376, 128, 376, "relu"),   # Humanoid: N above the hidden width, K no multiple of 32
          (64, 324, 256, 2, "tanh"),     # visgrid: H at the limit, N of 2
          (16, 8, 64, 8, "none")]
IDS = [f"{m}x{k}-{h}-{n}-{a}" for m, k, h, n, a in SHAPES]
_CACHE = {}


def _problem(M, K, H, N, act):
    """inputs and the fp32-CPU / fp64 references of one shape, computed once and shared (never modified)"""
    key = (M, K, H, N, act)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 + M + 7 * K + 13 * H + 17 * N)
    r = lambda *s: torch.randn(*s, generator=g)
    p = dict(X=r(M, K), W0=r(H, K) / np.sqrt(K), b0=0.1 * r(H), W1=r(N, H) / np.sqrt(H), b1=0.1 * r(N), dY=r(M, N))
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        X, W0, b0, W1, b1 = (p[k].to(dt).clone().requires_grad_(k != "X") for k in ("X", "W0", "b0", "W1", "b1"))
        z0 = F.linear(X, W0, b0)
        h = torch.relu(z0)
        z1 = F.linear(h, W1, b1)
        z0.retain_grad(); z1.retain_grad()
        y = mc.mlp2_act(act, z1)
        y.backward(p["dY"].to(dt))
        out[name] = dict(Y=y.detach(), H=h.detach(), dZ1=z1.grad, dZ0=z0.grad, gW0=W0.grad, gb0=b0.grad, gW1=W1.grad,
                         gb1=b1.grad)
    bounds = {k: mc.measured_bound(out["f32"][k], out["f64"][k]) for k in out["f64"]}
    _CACHE[key] = (p, out["f64"], bounds)
    return _CACHE[key]


def _check(name, got, want64, bound):
    err = float((got.double().cpu() - want64).abs().max())
    print(f"{name}: worst |kernel - fp64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


def _dev(p):
    return {k: v.cuda().contiguous() for k, v in p.items()}


@pytest.mark.parametrize("strided", [False, True], ids=["tight", "strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_forward_and_backward_per_element(shape, strided):
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    M, K, H, N, act = shape
    p, ref, bounds = _problem(*shape)
    assert lib.ssac_enc_mlp2_covered(M, K, H, N) == 1
    d = _dev(p)
    st = engine.stream()
    ldx, ldy = (K + 5, N + 3) if strided else (K, N)
    Xb = torch.full((M, ldx), float("nan"), device="cuda")
    Xb[:, :K] = d["X"]
    Yb = torch.full((M, ldy), float("nan"), device="cuda")
    Hs = torch.empty(M, H, device="cuda")
    check(lib.ssac_enc_mlp2_fwd(Xb.data_ptr(), ldx, d["W0"].data_ptr(), d["b0"].data_ptr(), d["W1"].data_ptr(),
                                d["b1"].data_ptr(), M, K, H, N, ACT[act], Hs.data_ptr(), Yb.data_ptr(), ldy, st))
    _check("Y", Yb[:, :N], ref["Y"], bounds["Y"])
    _check("H_save", Hs, ref["H"], bounds["H"])
    assert bool(torch.isnan(Yb[:, N:]).all()), "columns beyond N were written"
    # without H_save: the same Y, bit for bit
    Y2 = torch.full((M, ldy), float("nan"), device="cuda")
    check(lib.ssac_enc_mlp2_fwd(Xb.data_ptr(), ldx, d["W0"].data_ptr(), d["b0"].data_ptr(), d["W1"].data_ptr(),
                                d["b1"].data_ptr(), M, K, H, N, ACT[act], 0, Y2.data_ptr(), ldy, st))
    assert torch.equal(Y2[:, :N], Yb[:, :N])
    ldd = N + 2 if strided else N
    dYb = torch.full((M, ldd), float("nan"), device="cuda")
    dYb[:, :N] = d["dY"]
    dZ1 = torch.full((M, N), float("nan"), device="cuda")
    dZ0 = torch.full((M, H), float("nan"), device="cuda")
    check(lib.ssac_enc_mlp2_bwd(dYb.data_ptr(), ldd, Yb.data_ptr(), ldy, Hs.data_ptr(), d["W1"].data_ptr(), M, H, N,
                                ACT[act], dZ1.data_ptr(), dZ0.data_ptr(), st))
    _check("dZ1", dZ1, ref["dZ1"], bounds["dZ1"])
    _check("dZ0", dZ0, ref["dZ0"], bounds["dZ0"])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_activation_passes_per_element(shape):
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    M, K, H, N, act = shape
    p, ref, bounds = _problem(*shape)
    st = engine.stream()
    # the pre-activation in fp32 (its own rounding is inside the measured bound of Y)
    z1 = F.linear(torch.relu(F.linear(p["X"], p["W0"], p["b0"])), p["W1"], p["b1"])
    Yb = torch.full((M, N + 3), float("nan"), device="cuda")
    Yb[:, :N] = z1.cuda()
    check(lib.ssac_enc_act_fwd(Yb.data_ptr(), N + 3, M, N, ACT[act], st))
    _check("act(Y)", Yb[:, :N], ref["Y"], bounds["Y"])
    assert bool(torch.isnan(Yb[:, N:]).all())
    dZ = torch.empty(M, N, device="cuda")
    dY = p["dY"].cuda()
    check(lib.ssac_enc_act_bwd(dY.data_ptr(), N, Yb.data_ptr(), N + 3, M, N, ACT[act], dZ.data_ptr(), st))
    _check("act'(Y) dY", dZ, ref["dZ1"], bounds["dZ1"])


def _engine_for(shape, fused):
    import super_sac_amd as ssa
    from super_sac_amd import mlp_encoder as me
    M, K, H, N, act = shape
    p, ref, bounds = _problem(*shape)
    enc = ssa.nets.MlpEncoder(K, H, N, out_act=act)
    with torch.no_grad():
        enc.fc1.weight.copy_(p["W0"]); enc.fc1.bias.copy_(p["b0"])
        enc.fc2.weight.copy_(p["W1"]); enc.fc2.bias.copy_(p["b1"])
    enc = enc.cuda()
    me.USE_FUSED = "all" if fused else False   # ("all": both fused launches wherever the shape is covered)
    eng = me.mlp_engine(enc, torch.device("cuda"))
    covered = bool(me.lib.ssac_enc_mlp2_covered(M, K, H, N))
    assert eng.is_bound() and eng.fused(M) == eng.fused_backward(M) == (fused and covered)
    return enc, eng


def _engine_pass(shape, fused, A=3):
    from super_sac_amd import mlp_encoder as me
    M, K, H, N, act = shape
    p, ref, bounds = _problem(*shape)
    saved = me.USE_FUSED
    try:
        enc, eng = _engine_for(shape, fused)
        xin = torch.full((M, N + A), float("nan"), device="cuda")
        eng.forward(p["X"].cuda(), xin, N + A, True)
        eng.backward(p["dY"].cuda().contiguous())
        torch.cuda.synchronize()
        return xin, {k: eng._seg(i, eng.grads).clone().view(eng.plist[i].shape)
                     for i, k in enumerate(("gW0", "gb0", "gW1", "gb1"))}, eng
    finally:
        me.USE_FUSED = saved


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_engine_gradients_in_both_forms(shape):
    M, K, H, N, act = shape
    p, ref, bounds = _problem(*shape)
    outs = {}
    for fused in (True, False):
        xin, g, eng = _engine_pass(shape, fused)
        tag = "fused" if fused else "layers"
        _check(f"{tag} Y", xin[:, :N], ref["Y"], bounds["Y"])
        assert bool(torch.isnan(xin[:, N:]).all())
        for k in ("gW0", "gb0", "gW1", "gb1"):
            _check(f"{tag} {k}", g[k], ref[k], bounds[k])
        outs[fused] = (xin[:, :N].clone(), g)
    # the two forms against each other, under the same bound
    assert float((outs[True][0] - outs[False][0]).abs().max()) <= bounds["Y"]
    for k in ("gW0", "gb0", "gW1", "gb1"):
        assert float((outs[True][1][k] - outs[False][1][k]).abs().max()) <= bounds[k], k


def test_the_default_takes_the_fused_forward_where_it_measured_faster():
    """ssac_enc_mlp2_supported (profiles/mlp_encoder.md): one K chunk; the engine's default follows it"""
    from super_sac_amd import mlp_encoder as me
    from super_sac_amd._lib import lib
    assert me.USE_FUSED is True
    assert lib.ssac_enc_mlp2_supported(256, 17, 128, 17) == 1 and lib.ssac_enc_mlp2_supported(1, 11, 128, 11) == 1
    assert lib.ssac_enc_mlp2_supported(256, 376, 128, 376) == 0 and lib.ssac_enc_mlp2_covered(256, 376, 128, 376) == 1
    assert lib.ssac_enc_mlp2_supported(256, 324, 256, 2) == 0 and lib.ssac_enc_mlp2_covered(256, 324, 256, 2) == 1


@pytest.mark.parametrize("H", [48, 512])
def test_uncovered_hidden_widths_run_per_layer(H):
    from super_sac_amd._lib import lib
    shape = (37, 17, H, 17, "relu")
    M, K, _, N, act = shape
    assert lib.ssac_enc_mlp2_supported(M, K, H, N) == 0 and lib.ssac_enc_mlp2_covered(M, K, H, N) == 0
    p, ref, bounds = _problem(*shape)
    xin, g, eng = _engine_pass(shape, True)
    assert not eng.saved["fused"] and not eng.saved["fused_bwd"]
    _check("Y", xin[:, :N], ref["Y"], bounds["Y"])
    for k in ("gW0", "gb0", "gW1", "gb1"):
        _check(k, g[k], ref[k], bounds[k])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
def test_the_same_pass_twice_is_bit_identical(fused):
    shape = (300, 17, 128, 17, "relu")    # several row tiles and several weight-gradient slices
    x1, g1, _ = _engine_pass(shape, fused)
    x2, g2, _ = _engine_pass(shape, fused)
    assert torch.equal(x1[:, :17], x2[:, :17])
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_accumulate_adds_to_the_gradient_arena():
    from super_sac_amd import mlp_encoder as me
    shape = SHAPES[2]
    p, ref, bounds = _problem(*shape)
    saved = me.USE_FUSED
    try:
        enc, eng = _engine_for(shape, True)
    finally:
        me.USE_FUSED = saved
    out = torch.empty(shape[0], shape[3], device="cuda")
    eng.forward(p["X"].cuda(), out, shape[3], True)
    dY = p["dY"].cuda().contiguous()
    eng.backward(dY)
    once = eng.grads.clone()
    eng.backward(dY, accumulate=True)
    assert torch.equal(eng.grads, once + once)
