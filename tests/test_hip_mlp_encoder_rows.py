"""GPU: the few-row forward of the MLP encoder (ssac_enc_mlp2_fwd_rows, csrc/ssac_enc_mlp.hip), per element against fp64.

The tolerance is the project's measured rule (mlp_encoder_cases.measured_bound): 4 x the largest distance between torch's
own fp32 CPU result and the fp64 result on the same inputs, never below one fp32 ulp of the largest magnitude involved.
The launch hands layer 2 to the last workgroup to arrive; which one that is must not show: the same inputs twice, and 200
launches back to back on one scratch block (the arrival counter has to come back to zero every time), give equal bits.

Worst |kernel - fp64| / bound measured on an MI355X: see profiles/mlp_encoder.md ("Acting").
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_encoder_cases as mc

pytestmark = pytest.mark.gpu

ACT = {"none": 0, "relu": 1, "tanh": 2}
ROWS = [1, 3, 16]
SHAPES = [(3, 32, 2, "tanh"),         # K below one 16-byte chunk, the smallest hidden width, N of 2: 64 lanes per column
          (33, 128, 11, "relu"),      # K and N no multiple of 4: W0 rows of every alignment
          (324, 256, 2, "tanh"),      # visgrid: H at the limit, two K passes of a wave
          (376, 128, 376, "relu"),    # Humanoid: N above one pass of layer 2
          (17, 64, 33, "none")]       # SharedEncoder-sized K, 4 lanes per column would not fit: 8, two passes
IDS = [f"{k}-{h}-{n}-{a}" for k, h, n, a in SHAPES]
SCRATCH = 4 + 16 * 256                # SSAC_ENC_ROWS_SCRATCH
_CACHE = {}


def _problem(M, K, H, N, act):
    """inputs and the fp64 reference with its measured bound, computed once and shared (never modified)"""
    key = (M, K, H, N, act)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(2000 + M + 7 * K + 13 * H + 17 * N)
        r = lambda *s: torch.randn(*s, generator=g)
        p = dict(X=r(M, K), W0=r(H, K) / np.sqrt(K), b0=0.1 * r(H), W1=r(N, H) / np.sqrt(H), b1=0.1 * r(N))
        ys = {}
        for dt in (torch.float32, torch.float64):
            q = {k: v.to(dt) for k, v in p.items()}
            ys[dt] = mc.mlp2_act(act, F.linear(torch.relu(F.linear(q["X"], q["W0"], q["b0"])), q["W1"], q["b1"]))
        _CACHE[key] = (p, ys[torch.float64], mc.measured_bound(ys[torch.float32], ys[torch.float64]))
    return _CACHE[key]


def _offset(t, floats):
    """a copy of `t` whose storage starts `floats` floats behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _launch(p, M, K, H, N, act, ldx=None, ldy=None, x_offset=0, scratch=None, w_offset=0):
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    ldx, ldy = ldx or K, ldy or N
    d = {k: _offset(v.cuda().contiguous(), w_offset) for k, v in p.items() if k != "X"}
    Xb = torch.full((M * ldx + 4,), float("nan"), device="cuda")
    Xv = Xb[x_offset:x_offset + M * ldx].view(M, ldx)
    Xv[:, :K] = p["X"].cuda()
    Yb = torch.full((M, ldy), float("nan"), device="cuda")
    scratch = torch.zeros(SCRATCH, device="cuda") if scratch is None else scratch
    check(lib.ssac_enc_mlp2_fwd_rows(Xv.data_ptr(), ldx, d["W0"].data_ptr(), d["b0"].data_ptr(), d["W1"].data_ptr(),
                                     d["b1"].data_ptr(), M, K, H, N, ACT[act], Yb.data_ptr(), ldy, scratch.data_ptr(),
                                     engine.stream()))
    torch.cuda.synchronize()
    return Yb, scratch


def _check(name, got, want64, bound):
    err = float((got.double().cpu() - want64).abs().max())
    print(f"{name}: worst |kernel - fp64| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_forward_per_element(shape, M):
    from super_sac_amd._lib import lib
    K, H, N, act = shape
    assert lib.ssac_enc_mlp2_rows_covered(M, K, H, N) == 1
    p, ref, bound = _problem(M, *shape)
    Y, scratch = _launch(p, M, K, H, N, act)
    _check(f"rows {M}x{K}-{H}-{N}-{act}", Y, ref, bound)
    assert int(scratch[:1].view(torch.int32)) == 0, "the arrival counter did not return to zero"
    # the same inputs again, on a scratch block of their own: equal bits
    Y2, _ = _launch(p, M, K, H, N, act)
    assert torch.equal(Y, Y2)


@pytest.mark.parametrize("M", ROWS)
def test_strides_and_an_input_pointer_off_the_16_byte_grid(M):
    K, H, N, act = SHAPES[1]
    p, ref, bound = _problem(M, K, H, N, act)
    tight, _ = _launch(p, M, K, H, N, act)
    Y, _ = _launch(p, M, K, H, N, act, ldx=K + 3, ldy=N + 5)
    _check("strided", Y[:, :N], ref, bound)
    assert bool(torch.isnan(Y[:, N:]).all()), "columns beyond N were written"
    assert torch.equal(Y[:, :N], tight)
    Y, _ = _launch(p, M, K, H, N, act, x_offset=1)
    _check("X offset by one float", Y, ref, bound)
    assert torch.equal(Y, tight)
    # weights and biases off the grid as well: the scalar loads take the same k order
    Y, _ = _launch(p, M, K, H, N, act, w_offset=1)
    _check("weights offset by one float", Y, ref, bound)
    assert torch.equal(Y, tight)


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=[IDS[2], IDS[3]])
def test_200_launches_on_one_scratch_block_give_the_bits_of_the_first(shape):
    from super_sac_amd import engine
    from super_sac_amd._lib import check, lib
    K, H, N, act = shape
    M = 3
    p, ref, bound = _problem(M, *shape)
    d = {k: v.cuda().contiguous() for k, v in p.items()}
    scratch = torch.zeros(SCRATCH, device="cuda")
    Y = torch.full((200, M, N), float("nan"), device="cuda")
    st = engine.stream()
    for i in range(200):
        check(lib.ssac_enc_mlp2_fwd_rows(d["X"].data_ptr(), K, d["W0"].data_ptr(), d["b0"].data_ptr(), d["W1"].data_ptr(),
                                         d["b1"].data_ptr(), M, K, H, N, ACT[act], Y[i].data_ptr(), N, scratch.data_ptr(), st))
    torch.cuda.synchronize()
    _check("first of 200", Y[0], ref, bound)
    assert bool((Y == Y[0]).all()), "a later launch differs from the first: the counter or the hidden rows leaked"
    assert int(scratch[:1].view(torch.int32)) == 0


def test_the_launcher_refuses_what_it_does_not_cover():
    from super_sac_amd import engine
    from super_sac_amd._lib import lib
    K, H, N, act = SHAPES[4]
    # (buffers large enough for every shape asked for: a launch that went out by mistake stays inside them)
    X, W0, b0 = torch.zeros(17, K, device="cuda"), torch.zeros(512, K, device="cuda"), torch.zeros(512, device="cuda")
    W1, b1, Y = torch.zeros(N, 512, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(17, N, device="cuda")
    scratch = torch.zeros(4 + 17 * 512, device="cuda")
    for M_, H_ in ((17, H), (16, 48), (0, H), (16, 512)):
        assert lib.ssac_enc_mlp2_rows_covered(M_, K, H_, N) == 0
        rc = lib.ssac_enc_mlp2_fwd_rows(X.data_ptr(), K, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(), M_, K, H_,
                                        N, ACT[act], Y.data_ptr(), N, scratch.data_ptr(), engine.stream())
        assert rc != 0
        assert b"ssac_enc_mlp2_fwd_rows: shape not covered" in lib.ssac_last_error()
    torch.cuda.synchronize()
    assert lib.ssac_enc_mlp2_rows_covered(16, 513, H, N) == 0 and lib.ssac_enc_mlp2_rows_covered(16, 512, H, N) == 1
    for ldx, ldy in ((K - 1, N), (K, N - 1)):
        rc = lib.ssac_enc_mlp2_fwd_rows(X.data_ptr(), ldx, W0.data_ptr(), b0.data_ptr(), W1.data_ptr(), b1.data_ptr(), 16, K, H,
                                        N, ACT[act], Y.data_ptr(), ldy, scratch.data_ptr(), engine.stream())
        assert rc != 0 and b"bad stride" in lib.ssac_last_error()
    torch.cuda.synchronize()


def test_supported_implies_covered():
    from super_sac_amd._lib import lib
    for M in (0, 1, 2, 4, 5, 16, 17):
        for K in (1, 3, 17, 32, 33, 324, 376, 512, 513):
            for H in (32, 48, 64, 128, 256, 288):
                for N in (1, 2, 17, 376, 70000):
                    if lib.ssac_enc_mlp2_rows_supported(M, K, H, N):
                        assert lib.ssac_enc_mlp2_rows_covered(M, K, H, N), (M, K, H, N)


def test_the_default_takes_the_rows_form_where_it_measured_faster():
    """ssac_enc_mlp2_rows_supported (profiles/mlp_encoder.md, "Acting"): the measured K range 324 .. 376 only -- up to 4 rows
    into at most 4 outputs (visgrid), one row at H <= 128 (the Humanoid-sized shape); the engine's default follows it"""
    from super_sac_amd import mlp_encoder as me
    from super_sac_amd._lib import lib
    sup = lib.ssac_enc_mlp2_rows_supported
    assert me.USE_ROWS is True
    assert sup(1, 324, 256, 2) == 1 and sup(4, 324, 256, 2) == 1 and sup(1, 376, 128, 376) == 1
    assert sup(4, 376, 128, 376) == 0 and sup(5, 324, 256, 2) == 0 and sup(16, 324, 256, 2) == 0
    assert sup(1, 17, 128, 17) == 0 and sup(4, 17, 128, 17) == 0 and sup(1, 11, 128, 11) == 0   # (K <= 32: the fused tile launch)
    assert sup(1, 323, 256, 2) == 0 and sup(1, 377, 128, 2) == 0 and sup(1, 376, 256, 376) == 0   # (not measured: off)


def test_the_engine_takes_the_rows_form_only_without_save():
    import super_sac_amd as ssa
    from super_sac_amd import mlp_encoder as me
    M = 3
    K, H, N, act = SHAPES[1]
    p, ref, bound = _problem(M, K, H, N, act)
    enc = ssa.nets.MlpEncoder(K, H, N, out_act=act)
    with torch.no_grad():
        enc.fc1.weight.copy_(p["W0"]); enc.fc1.bias.copy_(p["b0"])
        enc.fc2.weight.copy_(p["W1"]); enc.fc2.bias.copy_(p["b1"])
    enc = enc.cuda()
    saved = me.USE_ROWS
    try:
        me.USE_ROWS = "all"
        eng = me.mlp_engine(enc, torch.device("cuda"))
        assert eng.rows(M) and not eng.rows(17)
        out = torch.full((M, N), float("nan"), device="cuda")
        eng.forward(p["X"].cuda(), out, N, False)
        assert ("t.rows", (SCRATCH,), torch.float32) in eng.ws._bufs, "the forward did not take the few-row launch"
        _check("engine, rows form", out, ref, bound)
        eng.saved = None
        kept = torch.full((M, N), float("nan"), device="cuda")
        eng.forward(p["X"].cuda(), kept, N, True)          # an update's forward keeps its form and what backward needs
        assert eng.saved is not None and eng.saved["h"].shape == (M, H)
        _check("engine, save=True", kept, ref, bound)
        me.USE_ROWS = False
        assert not eng.rows(M)
    finally:
        me.USE_ROWS = saved
