"""GPU: ssac_adv_candidates (csrc/ssac_adv.hip) -- the advantage estimator's stacked batch in one launch -- against the
sequence it stands in for inside a recorded critic update, on the same inputs and BIT FOR BIT:

  state copy into every block + data action into block 0 (two torch copies), then per sample
  tanh-normal head     ssac_tanh_normal_fwd into the block's action columns
  deterministic head   ssac_det_action_fwd (no draw: n equal candidates)

The Philox path (eps == NULL) is held to the same launch fed a buffer that ssac_philox_normal wrote under the documented
key (seed ^ SALT) and draw number.  X sits in a buffer with sentinel words behind it, which must survive; the inputs have
padded row strides whose padding is NaN, which must never be read.

Against fp64: the formulas restated in float64 on the host, per element.  The tolerance is derived here, not measured
(tests/test_hip_explore_action.py holds ssac_explore_action to the kernels it replaces bit for bit and has no fp64
bound to borrow).  With EPS = 2^-23, lo = -5, hi = 2: t = tanhf(raw) is within 2 ulp, so t + 1 (at most 2) carries at
most 3 EPS; times 0.5 (hi - lo) = 3.5 that is 10.5 EPS, the product's own rounding adds at most 3.5 EPS (value <= 7),
the sum with lo at most 2.5 EPS: |d log_std| <= 16.5 EPS < 20 EPS.  expf is within 2 ulp: sd has relative error <= 22
EPS, sd * e <= 22.5 EPS relative, the sum mu + sd e adds 0.5 EPS |u|, tanh has slope <= 1 and tanhf adds <= 2 EPS:
  |a - a64| <= EPS (22.5 |sd e| + 0.5 |u| + 2)  <  EPS (24 |sd e| + |u| + 4)       -- the bound asserted below;
the deterministic head and the copied columns: 4 EPS and 0."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (1, 3, 65)          # 65 straddles a wave
STATE = (1, 11, 16)
ACT = (1, 3, 6)
SAMPLES = (1, 4)
SALT = 0xADC0FFEE5A3B1E57   # the candidates' key salt (include/ssac_hip.h: ssac_adv_candidates)
EXPLORE_SALT = 0xE5A1C0DE0D15EA5E
SENTINEL = 7.5
LO, HI = -5.0, 2.0
GUARD = 64
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _padded(rows, width, ld, g, scale=1.0):
    t = torch.full((rows, ld), float("nan"))
    t[:, :width] = scale * torch.randn(rows, width, generator=g)
    return t.to(DEV)


def _inputs(rows, S, ld_s, A, n, tanh_normal, seed):
    g = torch.Generator().manual_seed(seed)
    width = 2 * A if tanh_normal else A
    s = _padded(rows, S, ld_s, g)
    act = _padded(rows, A, A + 2, g, 0.5)
    out = _padded(rows, width, width + 5, g, 1.5)
    eps = torch.randn(n * rows, A, generator=g).to(DEV)
    return s, act, out, eps


def _x(rows, S, A, n):
    return torch.full(((n + 1) * rows * (S + A) + GUARD,), SENTINEL, device=DEV)


def _candidates(ssa, s, S, act, A, out, tanh_normal, eps, rng, rows, n, X):
    return ssa._lib.lib.ssac_adv_candidates(
        s.data_ptr(), s.stride(0), act.data_ptr(), act.stride(0), out.data_ptr(), out.stride(0), int(tanh_normal),
        LO if tanh_normal else 0.0, HI if tanh_normal else 0.0, 0 if eps is None else eps.data_ptr(),
        0 if rng is None else C.addressof(rng), rows, S, A, n, X.data_ptr(), ssa.engine.stream())


def _present_sequence(ssa, s, S, act, A, out, tanh_normal, eps, rows, n, X):
    """adv_estimator.AdvantageEstimator.evaluate's stacked batch as it is assembled outside a critic update"""
    lib, st = ssa._lib.lib, ssa.engine.stream()
    W = S + A
    Xv = X[:(n + 1) * rows * W].view(n + 1, rows, W)
    Xv[:, :, :S].copy_(s[:, :S].unsqueeze(0).expand(n + 1, rows, S))
    Xv[0, :, S:].copy_(act[:, :A])
    for k in range(n):
        blk = Xv[k + 1]
        if tanh_normal:
            ssa._lib.check(lib.ssac_tanh_normal_fwd(out.data_ptr(), out.stride(0), eps[k * rows:].data_ptr(), rows, A, LO, HI,
                                                    blk.data_ptr(), W, S, 0, st))
        else:
            ssa._lib.check(lib.ssac_det_action_fwd(out.data_ptr(), out.stride(0), 0, 0.0, 0, 0.0, 0.0, rows, A,
                                                   blk.data_ptr(), W, S, st))


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _shapes():
    return itertools.product(ROWS, STATE, (0, 3), ACT)


@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_same_bits_as_the_present_sequence(ssa, head, n):
    tanh_normal = head == "tanh-normal"
    for j, (rows, S, pad, A) in enumerate(_shapes()):
        s, act, out, eps = _inputs(rows, S, S + pad, A, n, tanh_normal, 100 + j)
        ref, X = _x(rows, S, A, n), _x(rows, S, A, n)
        _present_sequence(ssa, s, S, act, A, out, tanh_normal, eps, rows, n, ref)
        ssa._lib.check(_candidates(ssa, s, S, act, A, out, tanh_normal, eps if tanh_normal else None, None, rows, n, X))
        what = (head, n, rows, S, pad, A)
        assert _same_bits(X, ref), what
        body = X[:(n + 1) * rows * (S + A)]
        assert bool(torch.isfinite(body).all()) and bool((X[body.numel():] == SENTINEL).all()), what
        if tanh_normal and n > 1 and rows * A >= 3:
            Xv = body.view(n + 1, rows, S + A)
            assert not torch.equal(Xv[1, :, S:], Xv[2, :, S:]), what   # (the samples are not copies of each other)


@pytest.mark.parametrize("aligned", [True, False], ids=["16-byte-rows", "misaligned-base"])
@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_the_16_byte_state_path_and_its_way_out(ssa, head, aligned):
    """S, ld_s and S + A multiples of four floats: state rows travel as 16-byte units -- unless a base address is not
    16-byte aligned, which takes the float path; same bits either way (shapes beyond the issue's grid, whose S + A is
    never a multiple of four)"""
    tanh_normal = head == "tanh-normal"
    for j, (rows, S, pad, A, n) in enumerate(itertools.product(ROWS, (8, 16), (0, 4), (4, 8), SAMPLES)):
        s, act, out, eps = _inputs(rows + 1, S, S + pad, A, n, tanh_normal, 300 + j)
        if not aligned:
            s = s.flatten()[1:1 + rows * (S + pad)].view(rows, S + pad)   # base 4 bytes past a 16-byte boundary
            s[:, :S] = torch.randn(rows, S, generator=torch.Generator().manual_seed(j)).to(DEV)
            assert s.data_ptr() % 16 == 4
        else:
            s = s[:rows]
            assert s.data_ptr() % 16 == 0
        act, out, eps = act[:rows], out[:rows], eps[:n * rows].contiguous()
        ref, X = _x(rows, S, A, n), _x(rows, S, A, n)
        assert X.data_ptr() % 16 == 0
        _present_sequence(ssa, s, S, act, A, out, tanh_normal, eps, rows, n, ref)
        ssa._lib.check(_candidates(ssa, s, S, act, A, out, tanh_normal, eps if tanh_normal else None, None, rows, n, X))
        assert _same_bits(X, ref), (head, aligned, rows, S, pad, A, n)


@pytest.mark.parametrize("counter", [False, True], ids=["host-draw-number", "device-counter"])
def test_in_kernel_noise_is_the_documented_philox_stream(ssa, counter):
    """eps == NULL: element ((k - 1) n_rows + b, i) of draw offset + *counter under the key seed ^ SALT"""
    lib, st = ssa._lib.lib, ssa.engine.stream()
    seed = 0x0123456789ABCDEF % (2 ** 62)
    ctr = torch.tensor([11], dtype=torch.int64, device=DEV) if counter else None
    ctr_ptr, offset = (ctr.data_ptr(), 30) if counter else (0, 41)

    def field(key, off, rows, A, n):
        buf = torch.zeros(n * rows, A, device=DEV)
        r = ssa._lib.Rng(key, ctr_ptr, off)
        ssa._lib.check(lib.ssac_philox_normal(buf.data_ptr(), n * rows, A, C.byref(r), st))
        return buf

    for j, (rows, S, pad, A) in enumerate(_shapes()):
        for n in SAMPLES:
            s, act, out, _ = _inputs(rows, S, S + pad, A, n, True, 500 + j)
            eps = field(seed ^ SALT, offset, rows, A, n)
            ref, X = _x(rows, S, A, n), _x(rows, S, A, n)
            ssa._lib.check(_candidates(ssa, s, S, act, A, out, True, eps, None, rows, n, ref))
            rs = ssa._lib.Rng(seed, ctr_ptr, offset)
            ssa._lib.check(_candidates(ssa, s, S, act, A, out, True, None, rs, rows, n, X))
            what = (rows, S, pad, A, n)
            assert _same_bits(X, ref), what
            assert bool((X[(n + 1) * rows * (S + A):] == SENTINEL).all()), what
            # the next draw, the unsalted key and the exploration process's key give other candidates
            for key, off in ((seed ^ SALT, offset + 1), (seed, offset), (seed ^ EXPLORE_SALT, offset)):
                other, other_eps = _x(rows, S, A, n), field(key, off, rows, A, n)
                assert not bool((other_eps == eps).any()), (what, hex(key), off)
                ssa._lib.check(_candidates(ssa, s, S, act, A, out, True, other_eps, None, rows, n, other))
                if n * rows * A >= 6:   # (a lone action can saturate to the same +-1 under two draws)
                    assert not _same_bits(other, ref), (what, hex(key), off)
                W = S + A
                # (only the candidates' action columns differ)
                a_, b_ = other[:(n + 1) * rows * W].view(n + 1, rows, W), ref[:(n + 1) * rows * W].view(n + 1, rows, W)
                assert _same_bits(a_[:, :, :S].contiguous(), b_[:, :, :S].contiguous()) and _same_bits(a_[0], b_[0]), what


@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_against_the_formulas_in_float64(ssa, head):
    tanh_normal = head == "tanh-normal"
    for j, (rows, S, pad, A) in enumerate(_shapes()):
        for n in SAMPLES:
            s, act, out, eps = _inputs(rows, S, S + pad, A, n, tanh_normal, 700 + j)
            X = _x(rows, S, A, n)
            ssa._lib.check(_candidates(ssa, s, S, act, A, out, tanh_normal, eps if tanh_normal else None, None, rows, n, X))
            W = S + A
            got = X[:(n + 1) * rows * W].view(n + 1, rows, W).cpu()
            s64, a64, o64, e64 = s[:, :S].cpu().double(), act[:, :A].cpu().double(), out.cpu().double(), eps.cpu().double()
            what = (head, rows, S, pad, A, n)
            assert torch.equal(got[:, :, :S].double(), s64.unsqueeze(0).expand(n + 1, rows, S)), what
            assert torch.equal(got[0, :, S:].double(), a64), what
            for k in range(1, n + 1):
                if tanh_normal:
                    log_std = LO + 0.5 * (HI - LO) * (torch.tanh(o64[:, A:2 * A]) + 1.0)
                    sde = torch.exp(log_std) * e64[(k - 1) * rows:k * rows]
                    u = o64[:, :A] + sde
                    want, tol = torch.tanh(u), EPS32 * (24.0 * sde.abs() + u.abs() + 4.0)
                else:
                    want = torch.tanh(o64[:, :A])
                    tol = torch.full_like(want, 4.0 * EPS32)
                err = (got[k, :, S:].double() - want).abs()
                assert bool((err <= tol).all()), (what, k, float((err / tol).max()))


def test_refusals_and_empty_batches(ssa):
    lib = ssa._lib.lib
    buf = torch.zeros(1 << 16, device=DEV)
    p, st = buf.data_ptr(), ssa.engine.stream()
    rs = ssa._lib.Rng(5, 0, 0)
    good = dict(s=p, ld_s=8, act=p, ld_act=4, out=p, ld_out=8, tanh_normal=1, lo=LO, hi=HI, eps=p, rng=0, n_rows=4,
                state_dim=8, act_dim=4, n_samples=2, X=p + 4096, stream=st)
    cases = [
        (dict(s=0), "ssac_adv_candidates: null argument"),
        (dict(X=0), "ssac_adv_candidates: null argument"),
        (dict(act_dim=0), "ssac_adv_candidates: act_dim must be in [1, 256]"),
        (dict(act_dim=257, ld_out=514, ld_act=257), "ssac_adv_candidates: act_dim must be in [1, 256]"),
        (dict(n_samples=0), "ssac_adv_candidates: state_dim and n_samples must be positive"),
        (dict(ld_s=7), "ssac_adv_candidates: row strides do not cover the state / the action / the head output"),
        (dict(ld_act=3), "ssac_adv_candidates: row strides do not cover the state / the action / the head output"),
        (dict(ld_out=7), "ssac_adv_candidates: row strides do not cover the state / the action / the head output"),
        (dict(tanh_normal=0), "ssac_adv_candidates: the deterministic head takes no eps"),
        (dict(eps=0), "ssac_adv_candidates: noise without a buffer needs the Philox stream (rng)"),
    ]
    for change, text in cases:
        args = dict(good, **change)
        assert lib.ssac_adv_candidates(*args.values()) != 0, change
        assert lib.ssac_last_error().decode() == text, change
    assert lib.ssac_adv_candidates(*dict(good, eps=0, rng=C.addressof(rs)).values()) == 0
    assert lib.ssac_adv_candidates(*dict(good, n_rows=0).values()) == 0
    assert lib.ssac_adv_candidates(*dict(good, n_rows=-3).values()) == 0
    torch.cuda.synchronize()
    assert bool((buf[:1024] == 0).all())   # (the sources are untouched)
