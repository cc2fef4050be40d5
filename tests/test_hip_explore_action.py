"""GPU: ssac_explore_action (csrc/ssac_explore.hip) -- head, then exploration process, in one launch -- against the
kernel sequences it stands in for inside a recorded critic update, on the same inputs and BIT FOR BIT:

  deterministic head   ssac_det_action_fwd with noise
  tanh-normal head     ssac_tanh_normal_fwd followed by ssac_exploration_noise (log pi included)

Bit equality is the whole contract: a recorded update issues this launch where the eager update under a noise hook
issues those, and the two runs must not differ.  The Philox path (eps / noise == NULL) is held to the same launch fed
buffers that ssac_philox_normal wrote under the documented keys.  Every output sits in a buffer with a padded row
stride, foreign columns and sentinel words behind it, all of which must survive."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (1, 63, 65, 255, 256, 257, 1025)   # around the wavefront, the 256-thread workgroup and several workgroups
ACT = (1, 3, 4, 6, 17)                    # 256 % A == 0 and != 0 (idle tail threads), more than one Philox block per row
SALT = 0xE5A1C0DE0D15EA5E                 # EXPLORE_KEY_SALT (include/ssac_hip.h: ssac_explore_action)
SENTINEL = 7.5
LO, HI = -5.0, 2.0
GUARD = 64


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _inputs(rows, A, tanh_normal, seed):
    g = torch.Generator().manual_seed(seed)
    width = 2 * A if tanh_normal else A
    ld_out = width + 5                    # padded head output
    out = torch.full((rows, ld_out), float("nan"))
    out[:, :width] = 1.5 * torch.randn(rows, width, generator=g)
    eps = torch.randn(rows, A, generator=g)
    noise = torch.randn(rows, A, generator=g)
    return out.to(DEV), ld_out, eps.to(DEV), noise.to(DEV)


def _outputs(rows, ld_act):
    act = torch.full((rows * ld_act + GUARD,), SENTINEL, device=DEV)
    logp = torch.full((rows + GUARD,), SENTINEL, device=DEV)
    return act, logp


def _explore(ssa, out, ld_out, tanh_normal, eps, noise, rng, scale_ptr, scale, clip, rows, A, act, ld_act, col0, logp):
    ssa._lib.check(ssa._lib.lib.ssac_explore_action(
        out.data_ptr(), ld_out, int(tanh_normal), LO if tanh_normal else 0.0, HI if tanh_normal else 0.0,
        0 if eps is None else eps.data_ptr(), 0 if noise is None else noise.data_ptr(),
        0 if rng is None else C.addressof(rng), scale_ptr, scale, clip, rows, A, act.data_ptr(), ld_act, col0,
        0 if logp is None else logp.data_ptr(), ssa.engine.stream()))


def _old_kernels(ssa, out, ld_out, tanh_normal, eps, noise, scale, clip, rows, A, act, ld_act, col0, logp):
    lib, st = ssa._lib.lib, ssa.engine.stream()
    if tanh_normal:
        ssa._lib.check(lib.ssac_tanh_normal_fwd(out.data_ptr(), ld_out, eps.data_ptr(), rows, A, LO, HI, act.data_ptr(),
                                                ld_act, col0, logp.data_ptr(), st))
        ssa._lib.check(lib.ssac_exploration_noise(act.data_ptr(), ld_act, col0, noise.data_ptr(), scale, clip, rows, A, st))
    else:
        ssa._lib.check(lib.ssac_det_action_fwd(out.data_ptr(), ld_out, 0, 0.0, noise.data_ptr(), scale, clip, rows, A,
                                               act.data_ptr(), ld_act, col0, st))


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _untouched(act, logp, rows, A, ld_act, col0, wrote_logp):
    body = act[:rows * ld_act].view(rows, ld_act)
    assert bool((body[:, :col0] == SENTINEL).all()) and bool((body[:, col0 + A:] == SENTINEL).all())
    assert bool((act[rows * ld_act:] == SENTINEL).all())
    assert bool((logp[rows if wrote_logp else 0:] == SENTINEL).all())
    assert bool(torch.isfinite(body[:, col0:col0 + A]).all())


@pytest.mark.parametrize("A", ACT)
@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_same_bits_as_the_kernels_it_replaces(ssa, head, A):
    tanh_normal = head == "tanh-normal"
    for k, (rows, col0, clip) in enumerate(itertools.product(ROWS, (0, 9), (0.0, 0.3))):
        ld_act = col0 + A + 3
        scale = 0.7 if k % 3 else 0.05
        out, ld_out, eps, noise = _inputs(rows, A, tanh_normal, 100 + k)
        act_ref, logp_ref = _outputs(rows, ld_act)
        _old_kernels(ssa, out, ld_out, tanh_normal, eps, noise, scale, clip, rows, A, act_ref, ld_act, col0, logp_ref)
        # the scale is read from a device word: the by-value argument holds nonsense
        scale_dev = torch.tensor([scale], device=DEV)
        act, logp = _outputs(rows, ld_act)
        _explore(ssa, out, ld_out, tanh_normal, eps if tanh_normal else None, noise, None, scale_dev.data_ptr(), 99.0, clip,
                 rows, A, act, ld_act, col0, logp if tanh_normal else None)
        what = (head, rows, A, col0, clip)
        assert _same_bits(act, act_ref), what
        assert _same_bits(logp, logp_ref), what
        _untouched(act, logp, rows, A, ld_act, col0, tanh_normal)
        if clip and scale > 0.5 and rows * A >= 63:   # (the clip has bitten somewhere: P(|n| <= 0.43)^63 < 1e-30)
            assert bool((noise.abs() * scale > clip).any())
        if k % 4 == 0:
            # ... the by-value scale of eager callers gives the same bits, and log pi is optional
            act_v, logp_v = _outputs(rows, ld_act)
            _explore(ssa, out, ld_out, tanh_normal, eps if tanh_normal else None, noise, None, 0, scale, clip, rows, A,
                     act_v, ld_act, col0, None)
            assert _same_bits(act_v, act_ref), what
            assert bool((logp_v == SENTINEL).all()), what


@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_zero_scale_gives_the_clamped_head_output(ssa, head):
    tanh_normal = head == "tanh-normal"
    rows, A, col0 = 257, 6, 9
    ld_act = col0 + A + 3
    out, ld_out, eps, noise = _inputs(rows, A, tanh_normal, 7)
    out[:, :A] *= 8.0   # saturate some actions: tanh reaches +-1 in fp32 and the clamp has something to do
    lib, st = ssa._lib.lib, ssa.engine.stream()
    head_act, head_logp = _outputs(rows, ld_act)
    if tanh_normal:
        ssa._lib.check(lib.ssac_tanh_normal_fwd(out.data_ptr(), ld_out, eps.data_ptr(), rows, A, LO, HI,
                                                head_act.data_ptr(), ld_act, col0, head_logp.data_ptr(), st))
    else:
        ssa._lib.check(lib.ssac_det_action_fwd(out.data_ptr(), ld_out, 0, 0.0, 0, 0.0, 0.0, rows, A, head_act.data_ptr(),
                                               ld_act, col0, st))
    one, tiny = torch.tensor(1.0), torch.tensor(1e-6)
    want = head_act[:rows * ld_act].view(rows, ld_act)[:, col0:col0 + A].clamp(float(-one + tiny), float(one - tiny))
    assert bool((want != head_act[:rows * ld_act].view(rows, ld_act)[:, col0:col0 + A]).any()), "nothing was clamped"
    zero = torch.zeros(1, device=DEV)
    act, logp = _outputs(rows, ld_act)
    _explore(ssa, out, ld_out, tanh_normal, eps if tanh_normal else None, noise, None, zero.data_ptr(), 1.0, 0.3, rows, A,
             act, ld_act, col0, logp if tanh_normal else None)
    assert _same_bits(act[:rows * ld_act].view(rows, ld_act)[:, col0:col0 + A].contiguous(), want.contiguous())
    if tanh_normal:
        assert _same_bits(logp, head_logp)


@pytest.mark.parametrize("counter", [False, True], ids=["host-draw-number", "device-counter"])
@pytest.mark.parametrize("head", ["deterministic", "tanh-normal"])
def test_in_kernel_noise_is_the_documented_philox_stream(ssa, head, counter):
    """eps under the key `seed`, the process noise under seed ^ SALT, both element (b, i) of draw offset + *counter"""
    tanh_normal = head == "tanh-normal"
    lib, st = ssa._lib.lib, ssa.engine.stream()
    seed = 0x0123456789ABCDEF % (2 ** 62)
    ctr = torch.tensor([11], dtype=torch.int64, device=DEV) if counter else None
    ctr_ptr, offset = (ctr.data_ptr(), 30) if counter else (0, 41)
    for rows, A in ((1, 1), (65, 3), (257, 6), (1025, 17)):
        col0 = 9
        ld_act = col0 + A + 3
        out, ld_out, _, _ = _inputs(rows, A, tanh_normal, 3)
        eps, noise = torch.zeros(rows, A, device=DEV), torch.zeros(rows, A, device=DEV)
        r_eps, r_noise = ssa._lib.Rng(seed, ctr_ptr, offset), ssa._lib.Rng(seed ^ SALT, ctr_ptr, offset)
        ssa._lib.check(lib.ssac_philox_normal(eps.data_ptr(), rows, A, C.byref(r_eps), st))
        ssa._lib.check(lib.ssac_philox_normal(noise.data_ptr(), rows, A, C.byref(r_noise), st))
        if rows * A >= 195:
            assert float((eps.view(torch.int32) != noise.view(torch.int32)).float().mean()) > 0.99   # two fields, not one
        scale = torch.tensor([0.4], device=DEV)
        act_ref, logp_ref = _outputs(rows, ld_act)
        _explore(ssa, out, ld_out, tanh_normal, eps if tanh_normal else None, noise, None, scale.data_ptr(), 0.0, 0.3, rows,
                 A, act_ref, ld_act, col0, logp_ref if tanh_normal else None)
        act, logp = _outputs(rows, ld_act)
        _explore(ssa, out, ld_out, tanh_normal, None, None, r_eps, scale.data_ptr(), 0.0, 0.3, rows, A, act, ld_act, col0,
                 logp if tanh_normal else None)
        assert _same_bits(act, act_ref), (head, rows, A)
        assert _same_bits(logp, logp_ref), (head, rows, A)
        _untouched(act, logp, rows, A, ld_act, col0, tanh_normal)
        if tanh_normal:
            # one field from a buffer, the other from the stream
            act_m, logp_m = _outputs(rows, ld_act)
            _explore(ssa, out, ld_out, True, eps, None, r_eps, scale.data_ptr(), 0.0, 0.3, rows, A, act_m, ld_act, col0, logp_m)
            assert _same_bits(act_m, act_ref) and _same_bits(logp_m, logp_ref), (rows, A)


def test_refusals(ssa):
    lib = ssa._lib.lib
    buf = torch.zeros(4096, device=DEV)
    p, st = buf.data_ptr(), ssa.engine.stream()
    rs = ssa._lib.Rng(5, 0, 0)
    r = C.addressof(rs)
    good = dict(out=p, ld_out=8, tanh_normal=1, lo=LO, hi=HI, eps=p, noise=p, rng=0, scale_ptr=0, scale=0.1, clip=0.0,
                n_rows=4, act_dim=4, act_dst=p, ld_act=4, act_col0=0, logp=p, stream=st)
    cases = [
        (dict(out=0), "ssac_explore_action: null argument"),
        (dict(act_dst=0), "ssac_explore_action: null argument"),
        (dict(act_dim=0), "ssac_explore_action: act_dim must be in [1, 256]"),
        (dict(act_dim=257, ld_out=514, ld_act=257), "ssac_explore_action: act_dim must be in [1, 256]"),
        (dict(ld_out=7), "ssac_explore_action: row strides do not cover the head output / the action columns"),
        (dict(ld_act=3), "ssac_explore_action: row strides do not cover the head output / the action columns"),
        (dict(act_col0=1), "ssac_explore_action: row strides do not cover the head output / the action columns"),
        (dict(act_col0=-1), "ssac_explore_action: row strides do not cover the head output / the action columns"),
        (dict(tanh_normal=0), "ssac_explore_action: the deterministic head takes no eps and has no log pi"),
        (dict(tanh_normal=0, eps=0), "ssac_explore_action: the deterministic head takes no eps and has no log pi"),
        (dict(noise=0), "ssac_explore_action: a noise field without a buffer needs the Philox stream (rng)"),
        (dict(eps=0), "ssac_explore_action: a noise field without a buffer needs the Philox stream (rng)"),
    ]
    for change, text in cases:
        args = dict(good, **change)
        assert lib.ssac_explore_action(*args.values()) != 0, change
        assert lib.ssac_last_error().decode() == text, change
    assert lib.ssac_explore_action(*dict(good, noise=0, eps=0, rng=r).values()) == 0
    assert lib.ssac_explore_action(*dict(good, n_rows=0).values()) == 0
    assert lib.ssac_explore_action(*dict(good, n_rows=-3).values()) == 0
    torch.cuda.synchronize()
