"""GPU: the two kernels of csrc/ssac_members.hip through the C ABI.

ssac_members_sunrise_weights -- every weight of every member batch against a float64 reference written here, and bit for
bit against the pair of launches it replaces (ssac_ensemble_min_select per member, then ssac_sunrise_weights per batch) on
the same q; E in {2, 3, 5}, N in {1, 2}, B in {5, 64, 130} (below a wave, whole waves, a ragged tail), continuous (q_dim 1)
and discrete (q_dim 4, the taken action's column, read from a strided stacked batch), temperatures 1 and 20.
  per-element bound (the project's rule): 4 x the largest |torch float32 CPU - float64| over the case's weights, with a
  floor of one float32 ulp of the largest weight.  The four log words follow offline_head_cases.log_tol.
ssac_group_norms_pick -- bit for bit against ssac_group_norms on the picked buffer, for every pick at E = 3, with and
without the clip scale; group sizes 1, 160 and a ragged 1 484.
Every output is followed by sentinel words that must survive."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import offline_head_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _buf(numel):
    return torch.full((numel + oc.TAIL,), oc.SENT, device=DEV)


def _tail_ok(buf, numel, what):
    assert torch.equal(buf[numel:].cpu(), torch.full((oc.TAIL,), oc.SENT)), f"{what}: written past its end"


LD_ACT = 7   # row stride of the stacked batch the discrete case reads its actions from (column 3 of 7)
ACT_COL = 3


def _inputs(E, N, B, qd, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(E * N, E * B, qd, generator=g) * 1.7 + 0.3
    rows = None
    if qd > 1:
        rows = torch.full((E * B, LD_ACT), -3.0)   # (a column other than ACT_COL would select outside [0, qd))
        rows[:, ACT_COL] = torch.randint(0, qd, (E * B,), generator=g).float()
    return q, rows


def _reference(q, rows, E, N, B, qd, temp, dtype):
    """(E, B) weights in `dtype`, spelled as the reference does: min over a member's nets, the taken column, unbiased
    std over the members, sigmoid(-std * T) + 0.5 (learning_utils.py:372-382)"""
    q = q.to(dtype).view(E, N, E * B, qd).min(dim=1).values          # (member, stacked row, qd)
    if qd > 1:
        sel = rows[:, ACT_COL].long().view(1, E * B, 1).expand(E, E * B, 1)
        q = q.gather(-1, sel)
    std = q[..., 0].std(dim=0)                                        # (stacked row,)
    return (torch.sigmoid(-std * temp) + 0.5).view(E, B)


CASES = list(itertools.product((2, 3, 5), (1, 2), (5, 64, 130), (1, 4), (1.0, 20.0)))


@pytest.mark.parametrize("E,N,B,qd,temp", CASES)
def test_members_sunrise_weights(ssa, E, N, B, qd, temp):
    lib, chk, st = ssa._lib.lib, ssa._lib.check, ssa.engine.stream()
    q, rows = _inputs(E, N, B, qd, 1000 * E + 100 * N + B + qd)
    qd_, rows_d = q.to(DEV), (rows.to(DEV) if rows is not None else None)
    act_ptr = rows_d[:, ACT_COL:].data_ptr() if rows_d is not None else 0
    w, logs = _buf(E * B), _buf(4)
    chk(lib.ssac_members_sunrise_weights(qd_.data_ptr(), E, N, B, qd, temp, act_ptr, LD_ACT if rows is not None else 0,
                                         w.data_ptr(), logs.data_ptr(), st))
    torch.cuda.synchronize()
    _tail_ok(w, E * B, "w")
    _tail_ok(logs, 4, "logs")
    got = w[:E * B].view(E, B).cpu()
    # ---- float64, with the bound taken from torch's own float32 error on the same inputs
    ref64 = _reference(q, rows, E, N, B, qd, temp, F64)
    ref32 = _reference(q, rows, E, N, B, qd, temp, torch.float32)
    cpu_err = float((ref32.double() - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max())))
    bound = max(4.0 * cpu_err, ulp)
    err = float((got.double() - ref64).abs().max())
    print(f"E{E} N{N} B{B} qd{qd} T{temp}: max |kernel - f64| {err:.3g}, |torch f32 - f64| {cpu_err:.3g}, bound {bound:.3g}, "
          f"ratio {err / bound:.3g}")
    assert err <= bound
    last = ref64[E - 1]
    tol = oc.log_tol(last)
    for j, (name, want) in enumerate((("mean", last.mean()), ("max", last.max()), ("min", last.min()),
                                      ("std", last.std() if B > 1 else torch.zeros(())))):
        assert abs(float(logs[j]) - float(want)) <= tol, (name, float(logs[j]), float(want), tol)
    # ---- the pair of launches it replaces, on the same q: the same bits
    for i in range(E):
        qmin = torch.empty(E, B, device=DEV)
        for k in range(E):
            qk = qd_[k * N:(k + 1) * N, i * B:(i + 1) * B].contiguous()
            a_i = rows_d[i * B:(i + 1) * B, ACT_COL:] if rows_d is not None else None
            chk(lib.ssac_ensemble_min_select(qk.data_ptr(), N, B, qd, a_i.data_ptr() if a_i is not None else 0,
                                             LD_ACT if a_i is not None else 0, qmin[k].data_ptr(), st))
        w_i, logs_i = _buf(B), _buf(4)
        chk(lib.ssac_sunrise_weights(qmin.data_ptr(), E, B, temp, w_i.data_ptr(), logs_i.data_ptr(), st))
        torch.cuda.synchronize()
        assert torch.equal(w_i[:B].cpu(), got[i]), f"member batch {i}: not the bits of min_select + sunrise_weights"
    assert torch.equal(logs_i[:4].cpu(), logs[:4].cpu()), "log words: not the last member's, bit for bit"


def test_members_sunrise_weights_refusals(ssa):
    lib = ssa._lib.lib
    q, w = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    assert lib.ssac_members_sunrise_weights(q.data_ptr(), 1, 1, 4, 1, 1.0, 0, 0, w.data_ptr(), 0, ssa.engine.stream()) != 0
    assert lib.ssac_members_sunrise_weights(q.data_ptr(), 9, 1, 4, 1, 1.0, 0, 0, w.data_ptr(), 0, ssa.engine.stream()) != 0
    assert lib.ssac_members_sunrise_weights(q.data_ptr(), 2, 1, 4, 4, 1.0, 0, 0, w.data_ptr(), 0, ssa.engine.stream()) != 0
    assert b"ssac_members_sunrise_weights" in lib.ssac_last_error()


@pytest.mark.parametrize("clip", (False, True))
@pytest.mark.parametrize("group_size", (1, 160, 1484))
def test_group_norms_pick(ssa, group_size, clip):
    lib, chk, st = ssa._lib.lib, ssa._lib.check, ssa.engine.stream()
    E, n_groups = 3, 2
    g = torch.Generator().manual_seed(group_size)
    bufs = [(torch.rand(n_groups * group_size, generator=g) * (k + 1) * 3.0).to(DEV) for k in range(E)]
    ctl = None
    if clip:
        ctl = ssa.engine.DeviceStruct(ssa._lib.AdamCtl(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, clip_coef=0.37109375),
                                      torch.device(DEV))
    table = (C.c_void_p * E)(*[b.data_ptr() for b in bufs])
    for pick in range(E):
        word = torch.tensor([7, pick, 7], dtype=torch.int32, device=DEV)   # (the word sits between two others)
        out, want = _buf(n_groups), _buf(n_groups)
        chk(lib.ssac_group_norms_pick(table, E, word[1:].data_ptr(), n_groups, group_size, ctl.ptr if ctl else 0,
                                      out.data_ptr(), st))
        chk(lib.ssac_group_norms(bufs[pick].data_ptr(), n_groups, group_size, ctl.ptr if ctl else 0, want.data_ptr(), st))
        torch.cuda.synchronize()
        _tail_ok(out, n_groups, "out")
        assert torch.equal(out.cpu(), want.cpu()), f"pick {pick}: not ssac_group_norms' bits"
        ref = bufs[pick].double().view(n_groups, group_size).sum(1).sqrt() * (0.37109375 if clip else 1.0)
        assert torch.allclose(out[:n_groups].double().cpu(), ref.cpu(), rtol=1e-5, atol=0)
    # a word outside [0, E) is clamped, never followed outside the table
    word = torch.tensor([E + 5], dtype=torch.int32, device=DEV)
    out = _buf(n_groups)
    chk(lib.ssac_group_norms_pick(table, E, word.data_ptr(), n_groups, group_size, 0, out.data_ptr(), st))
    want = _buf(n_groups)
    chk(lib.ssac_group_norms(bufs[E - 1].data_ptr(), n_groups, group_size, 0, want.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want.cpu())
