"""Seeded inputs and float64 references for the offline-update and weighting row kernels of csrc/ssac_elementwise.hip and
csrc/ssac_markov.hip: ssac_adv_filter(_discrete), ssac_bc_logprob_bwd, ssac_bc_discrete_bwd, ssac_bc_det_logprob_bwd,
ssac_action_invariance_det_bwd, ssac_actor_loss_bwd_adv, ssac_dr3_add, ssac_softmax_weights, ssac_sunrise_weights and
ssac_ensemble_min_select.  Helpers only, no tests and no GPU imports: tests/test_hip_offline_heads.py runs the kernels on
these inputs, tests/test_offline_head_cases_cpu.py proves the inputs and references fit for purpose without a kernel.

A case is a dict with an "id"; ``<kernel>_inputs(case)`` draws its float32 inputs (seeded by the id) and
``<kernel>_ref(inputs, case, dtype)`` evaluates the reference project's formula with torch in ``dtype`` -- float64 is the
reference, float32 the same formula at the kernels' precision.  Gradients come from torch.autograd.

Row counts: LADDER = a lone row, a partial and a just-full wave, the last row before the second trip of the
``b += blockDim.x`` loop (1024 threads), the boundary, one past it, and a third, partial trip.

Tolerances
----------
* index and selection work (mask, arg-min routing, min/select, the grid-input advantages, sentinels, what an all-zero mask
  leaves) is compared bit for bit.
* per element: |got - ref| <= atol + rtol |ref| with atol = 1e-7 * max|ref| of the case.  rtol is not picked from what the
  kernel gives: F32_DEV records, per kernel and case family, the worst deviation of the SAME formula in torch float32 on the
  CPU from the float64 reference (the smallest rtol that satisfies the bound above, over all cases of the family), and
  ``rtol(family) = max(1e-5, 4 * F32_DEV[family])``: the device's tanhf / expf / log1pf differ from the host's by a few ulp
  and the kernels add in another order, a wrong formula or stride misses by orders of magnitude; 1e-5 is the constant of the
  sibling tests in test_hip_kernels.py.  The CPU test asserts the measured deviation stays under F32_DEV.

  family                measured   F32_DEV   rtol
  adv_filter            3.6e-08    1e-07     1e-05     (n_samp 3 or a general PopArt map; rows nearer 0 than 1e-4 shifted away)
  adv_filter_discrete   2.4e-07    5e-07     1e-05
  bc_logprob_lo5        1.8e-06    4e-06     1.6e-05   ((r2 - 1) and (x - mu) cancel; log_std in [-5, 2])
  bc_logprob_lo10       4.3e-06    9e-06     3.6e-05   (log_std down to -10: exp() amplifies the rounding of tanh)
  bc_discrete_x1.5      6.8e-08    2e-07     1e-05
  bc_discrete_x20       1.3e-03    2.5e-03   1e-02     (saturated softmax: torch's onehot - p cancels to ~2 atol where p -> 1)
  bc_det                1.0e-07    2.5e-07   1e-05     (|a - loc| >= 0.05, |out| <= 1.5: nothing cancels)
  actinv_det            2.0e-07    4e-07     1e-05
  actor_adv             0          1e-07     1e-05     (a constant per routed element)
  dr3                   0          1e-07     1e-05     (one product and one add per element)
  softmax_t1            2.3e-08    2e-07     1e-05     (std spelled out in float32 ops: _std0)
  softmax_t20           0          2e-07     1e-05
  softmax_t2000         0          1e-07     1e-05     (one or two rows hold all the weight, the rest lies under atol)
  sunrise_t20           0          1e-07     1e-05

  (measured: this module's cases, torch CPU float32; most of the float32 error lies under atol, hence the small figures.
  F32_DEV leaves about 2 x for another libm.)
* reduced log words: |got - ref| <= 1e-5 * mean_b|term_b| + 1e-6 (log_tol): at most 3 serial adds per thread, 6 shuffle steps
  and 16 wave partials are ~25 roundings, ~1.5e-6 of sum|term|; the constant of test_critic_loss_bwd_*.  The max / min words of
  the weight kernels are selections of per-element values and take the per-element bound; their std word adds to log_tol what
  the per-element bound lets through: std is 1-Lipschitz in the root-mean-square norm, so a perturbation |d_b| <= atol + rtol
  |w_b| moves it by at most sqrt(n / (n - 1)) * (atol + rtol * rms(w)) (std_tol).
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import ssac_oracle as orc

F64, F32 = torch.float64, torch.float32
LADDER = (1, 63, 65, 1023, 1024, 1025, 2500)
SENT = -777.25            # what padding columns and the words past every output hold before the launch
TAIL = 8                  # sentinel words past each output
PRE = 0.75                # what an accumulated log word holds before the launch
ACT_EDGES = (1.0, -1.0, 0.99, -0.99, 0.995, -0.995, 0.0)   # data actions at and beyond the atanh clamp


def _f32(x):
    return float(np.float32(x))


POP_EXACT = (0.5, 0.25)                       # exact on the 2^-6 grid
POP_GENERAL = (_f32(0.8371), _f32(-0.2113))   # (the device struct holds floats)

F32_DEV = {
    "adv_filter": 1e-7, "adv_filter_discrete": 5e-7, "bc_logprob_lo5": 4e-6, "bc_logprob_lo10": 9e-6,
    "bc_discrete_x1.5": 2e-7, "bc_discrete_x20": 2.5e-3, "bc_det": 2.5e-7, "actinv_det": 4e-7, "actor_adv": 1e-7,
    "dr3": 1e-7, "softmax_t1": 2e-7, "softmax_t20": 2e-7, "softmax_t2000": 1e-7, "sunrise_t20": 1e-7,
}


def rtol(family):
    return max(1e-5, 4.0 * F32_DEV[family])


def atol_of(ref):
    return 1e-7 * float(ref.abs().max())


def rel_dev(got, ref):
    """the smallest rtol with |got - ref| <= atol_of(ref) + rtol |ref| everywhere (inf: a miss where ref is 0)"""
    got, ref = got.detach().to(F64).reshape(-1), ref.detach().to(F64).reshape(-1)
    over = (got - ref).abs() - atol_of(ref)
    bad = over > 0
    if not bool(bad.any()):
        return 0.0
    return float((over[bad] / ref.abs()[bad]).max())


def log_tol(terms):
    return 1e-5 * float(terms.detach().to(F64).abs().mean()) + 1e-6


def std_tol(w, family):
    """the std word of the weight kernels: the reduction's share (the squared deviations are all positive, so log_tol's 1e-5
    of their sum is 1e-5 of the variance, half that of the std) plus what the per-element bound lets through"""
    n = w.numel()
    if n == 1:
        return 1e-6
    w = w.detach().to(F64)
    return 1e-5 * float(w.std()) + 1e-6 + math.sqrt(n / (n - 1.0)) * (atol_of(w) + rtol(family) * float(w.square().mean().sqrt()))


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["id"].encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _grid(g, *shape):
    """multiples of 2^-6 in [-8, 8]: min, sums of up to 5, halves and quarters of them are exact in float32"""
    return torch.randint(-512, 513, shape, generator=g).float() / 64.0


def _planted(n):
    """rows at the wave and trip boundaries"""
    return sorted({b for b in (0, 63, 64, 1023, 1024, n - 1) if 0 <= b < n})


def _fmt(v):
    if v is None or isinstance(v, tuple):
        return {None: "0", POP_EXACT: "exact", POP_GENERAL: "gen"}[v]
    return f"{v:g}" if isinstance(v, float) else str(v)


def _with_ids(prefix, cases):
    for c in cases:
        c["id"] = prefix + "-" + "-".join(k + _fmt(v) for k, v in c.items() if k != "family")
    return cases


def _mask(g, kind, n):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(n)
    return (torch.rand(n, generator=g) < 0.5).float()


def _padded(data, ld, fill=SENT):
    buf = torch.full((data.shape[0], ld), fill)
    buf[:, :data.shape[1]] = data
    return buf


def _index_column(idx, ld, n_classes):
    """the action index as float in column 0; further columns hold OTHER valid indices (a wrong stride reads a wrong class,
    never memory out of bounds)"""
    buf = torch.empty(idx.numel(), ld)
    for c in range(ld):
        buf[:, c] = ((idx + c) % n_classes).float()
    return buf


# ------------------------------------------------------------------------------------------------ ssac_adv_filter
def _af(n, nets, samp, use_max, popart, exact, null=None):
    return dict(n=n, nets=nets, samp=samp, max=use_max, popart=popart, exact=exact, null=null, family="adv_filter")


ADV_FILTER = _with_ids("af", [
    _af(1, 1, 1, 0, None, True), _af(63, 3, 4, 0, POP_EXACT, True), _af(65, 3, 4, 1, None, True),
    _af(1024, 1, 4, 0, POP_EXACT, True, "adv"), _af(1025, 3, 1, 1, POP_EXACT, True), _af(2500, 3, 4, 0, None, True),
    _af(1, 3, 4, 0, POP_GENERAL, False), _af(65, 3, 3, 0, POP_GENERAL, False), _af(1023, 1, 3, 1, None, False, "mask"),
    _af(1025, 3, 3, 0, None, False, "prio"), _af(2500, 3, 3, 1, POP_GENERAL, False), _af(2500, 1, 4, 0, POP_GENERAL, False),
])


def adv_filter_inputs(case):
    g = _gen(case)
    n, N, S = case["n"], case["nets"], case["samp"]
    if case["exact"]:
        q = _grid(g, N, 1 + S, n)
        for b in _planted(n):
            q[:, :, b] = q[0, 0, b]    # every Q of the row equal: the advantage is exactly 0 under min / mean / max / w q + b
    else:
        q = _randn(g, N, 1 + S, n) * 2.0
        near = adv_filter_ref(dict(q=q), case)["adv"].abs() < 1e-4
        q[:, 0, near] += 0.5           # no row near the threshold of the mask
    return dict(q=q.reshape(N, -1).contiguous())


def adv_filter_ref(inp, case, dtype=F64):
    """adv_estimator.py:58-79, learning_utils.py:254-256, 293"""
    q = inp["q"].to(dtype).view(case["nets"], 1 + case["samp"], case["n"])
    mq = q.min(0).values
    if case["popart"]:
        mq = case["popart"][0] * mq + case["popart"][1]
    value = mq[1:].max(0).values if case["max"] else mq[1:].mean(0)
    adv = mq[0] - value
    mask = (adv >= 0.0).to(dtype)
    return dict(adv=adv, mask=mask, prio=F.relu(adv) + 1e-4, logs=mask.mean().reshape(1), terms=mask)


# ------------------------------------------------------------------------------------------------ ssac_adv_filter_discrete
def _afd(n, actors, nets, A, ld, popart, exact=False, null=None):
    return dict(n=n, actors=actors, nets=nets, A=A, ld=ld, popart=popart, exact=exact, null=null, family="adv_filter_discrete")


ADV_FILTER_DISCRETE = _with_ids("afd", [
    _afd(1, 1, 1, 2, 1, None), _afd(65, 2, 2, 6, 3, POP_GENERAL), _afd(1023, 1, 2, 18, 1, None),
    _afd(1024, 2, 2, 2, 1, POP_GENERAL, null="mask"), _afd(1025, 2, 1, 6, 1, POP_GENERAL, null="adv"),
    _afd(2500, 2, 2, 18, 3, None, null="prio"), _afd(1025, 2, 2, 2, 1, POP_EXACT, exact=True),
    _afd(65, 1, 2, 2, 3, None, exact=True),
])


def adv_filter_discrete_inputs(case):
    g = _gen(case)
    n, N, E, A = case["n"], case["nets"], case["actors"], case["A"]
    idx = torch.randint(0, A, (n,), generator=g)
    if case["exact"]:   # equal logits: both probabilities are exactly 1/2
        q = _grid(g, N, n, A)
        logits = _randn(g, E, n, 1).expand(E, n, A).contiguous()
        for b in _planted(n):
            q[:, b, :] = q[0, b, 0]
    else:
        q = _randn(g, N, n, A) * 2.0
        logits = _randn(g, E, n, A) * 1.5
        near = (adv_filter_discrete_ref(dict(q=q, logits=logits, idx=idx), case)["adv"].abs() < 1e-4).nonzero().squeeze(1)
        q[:, near, idx[near]] += 0.5
    return dict(q=q, logits=logits, idx=idx, act=_index_column(idx, case["ld"], A))


def adv_filter_discrete_ref(inp, case, dtype=F64):
    """adv_estimator.py:41-56"""
    probs = torch.softmax(inp["logits"].to(dtype), dim=-1).mean(0)
    mq = inp["q"].to(dtype).min(0).values
    if case["popart"]:
        mq = case["popart"][0] * mq + case["popart"][1]
    value = (probs * mq).sum(-1, keepdim=True)
    adv = (mq.gather(-1, inp["idx"][:, None]) - value)[:, 0]
    mask = (adv >= 0.0).to(dtype)
    return dict(adv=adv, mask=mask, prio=F.relu(adv) + 1e-4, logs=mask.mean().reshape(1), terms=mask)


# ------------------------------------------------------------------------------------------------ behavioural cloning heads
def _bc(n, A, pad, mask, inv, member=True, **kw):
    return dict(n=n, A=A, pad=int(pad), mask=mask, inv=inv, member=int(member), **kw)


def _bc_finish(lp, o, mask, inv, dtype):
    """learning_utils.py:264-267 for one member, and learning.py's sum over members / E"""
    w = torch.ones_like(lp) if mask is None else mask.to(dtype)
    terms = lp * w
    loss = -terms.mean()
    (loss * inv).backward()
    return dict(d_out=o.grad, member=loss.detach().reshape(1), total=(PRE + loss * inv).detach().reshape(1),
                terms=terms.detach())


BC_LOGPROB = _with_ids("bcl", [
    dict(_bc(1, 1, 0, "none", 1.0), lo=-5.0), dict(_bc(63, 6, 1, "rand", 0.5), lo=-10.0),
    dict(_bc(65, 17, 0, "zero", 1.0), lo=-5.0), dict(_bc(1023, 6, 1, "none", 10.0, member=False), lo=-10.0),
    dict(_bc(1024, 1, 1, "rand", 0.5), lo=-5.0), dict(_bc(1025, 17, 1, "rand", 1.0), lo=-10.0),
    dict(_bc(2500, 6, 0, "rand", 0.5), lo=-5.0), dict(_bc(2500, 1, 1, "zero", 10.0), lo=-10.0),
    dict(_bc(1, 6, 1, "none", 1.0), lo=-10.0),
])
for _c in BC_LOGPROB:
    _c["family"] = "bc_logprob_lo5" if _c["lo"] == -5.0 else "bc_logprob_lo10"
BC_HI = 2.0


def bc_strides(case, width):
    """(ld of the actor output, of the action, of the gradient)"""
    p = case["pad"]
    return width + 3 * p, case["A"] + 2 * p, width + 5 * p


def bc_logprob_inputs(case):
    g = _gen(case)
    n, A = case["n"], case["A"]
    ld_out, ld_act, _ = bc_strides(case, 2 * A)
    a = torch.tanh(_randn(g, n, A) * 1.5)
    k = min(len(ACT_EDGES), n * A)
    shift = zlib.crc32(case["id"].encode()) % len(ACT_EDGES)
    a.view(-1)[:k] = torch.tensor([ACT_EDGES[(i + shift) % len(ACT_EDGES)] for i in range(k)])
    return dict(out=_padded(_randn(g, n, 2 * A), ld_out), act=_padded(a, ld_act), mask=_mask(g, case["mask"], n))


def bc_logprob_ref(inp, case, dtype=F64):
    A = case["A"]
    o = inp["out"][:, :2 * A].to(dtype).clone().requires_grad_(True)
    lp = orc.tanh_normal_log_prob_data(o, case["lo"], BC_HI, inp["act"][:, :A].to(dtype))[:, 0]
    return _bc_finish(lp, o, inp["mask"], case["inv"], dtype)


BC_DISCRETE = _with_ids("bcd", [
    _bc(1, 2, 0, "none", 1.0, scale=1.5), _bc(65, 6, 1, "rand", 0.5, scale=20.0), _bc(1023, 18, 0, "zero", 1.0, scale=1.5),
    _bc(1024, 18, 0, "none", 0.5, scale=20.0), _bc(1025, 6, 1, "rand", 10.0, member=False, scale=1.5),
    _bc(2500, 18, 1, "rand", 1.0, scale=20.0), _bc(2500, 2, 0, "rand", 0.5, scale=1.5),
])
for _c in BC_DISCRETE:
    _c["family"] = "bc_discrete_x1.5" if _c["scale"] == 1.5 else "bc_discrete_x20"


def bc_discrete_inputs(case):
    g = _gen(case)
    n, A = case["n"], case["A"]
    idx = torch.randint(0, A, (n,), generator=g)
    return dict(logits=_randn(g, n, A) * case["scale"], idx=idx, act=_index_column(idx, 3 if case["pad"] else 1, A),
                mask=_mask(g, case["mask"], n))


def bc_discrete_ref(inp, case, dtype=F64):
    """learning_utils.py:257-268"""
    o = inp["logits"].to(dtype).clone().requires_grad_(True)
    lp = torch.log_softmax(o, dim=-1).gather(-1, inp["idx"][:, None])[:, 0]
    return _bc_finish(lp, o, inp["mask"], case["inv"], dtype)


# ---- deterministic actors: Normal(tanh(out), 1e-4).  With a variance of 1e-8 the heads are ill-conditioned wherever
# 1 - loc^2 or a - loc cancel; |out| <= 1.5 and |a - loc| >= 0.05 keep both away from that.
DET_OUT_MAX, DET_GAP = 1.5, 0.05


def _away_from(loc, a):
    """a, except where it lies within 0.075 of loc: there loc moved 0.075 towards 0"""
    moved = loc - torch.where(loc >= 0, 1.0, -1.0) * 1.5 * DET_GAP
    return torch.where((a - loc).abs() < 1.5 * DET_GAP, moved, a)


BC_DET = _with_ids("bcdet", [
    _bc(1, 1, 0, "none", 1.0), _bc(63, 17, 1, "rand", 0.5), _bc(65, 6, 1, "zero", 1.0),
    _bc(1024, 6, 0, "rand", 1.0, member=False), _bc(1025, 17, 1, "none", 0.5), _bc(2500, 1, 1, "rand", 10.0),
    _bc(2500, 6, 0, "rand", 1.0),
])
for _c in BC_DET:
    _c["family"] = "bc_det"


def bc_det_inputs(case):
    g = _gen(case)
    n, A = case["n"], case["A"]
    ld_out, ld_act, _ = bc_strides(case, A)
    out = (torch.rand(n, A, generator=g) * 2.0 - 1.0) * DET_OUT_MAX
    a = _away_from(torch.tanh(out), torch.rand(n, A, generator=g) * 2.0 - 1.0)
    return dict(out=_padded(out, ld_out), act=_padded(a, ld_act), mask=_mask(g, case["mask"], n))


def bc_det_ref(inp, case, dtype=F64):
    A = case["A"]
    o = inp["out"][:, :A].to(dtype).clone().requires_grad_(True)
    lp = orc.det_normal_log_prob(o, inp["act"][:, :A].to(dtype))[:, 0]
    return _bc_finish(lp, o, inp["mask"], case["inv"], dtype)


def _aid(n, A, pad, coeff, add_to=True):
    return dict(n=n, A=A, pad=int(pad), coeff=coeff, add=int(add_to), family="actinv_det")


ACTINV_DET = _with_ids("aid", [
    _aid(1, 1, 0, 1.0), _aid(65, 6, 1, 0.1), _aid(1023, 17, 0, 0.5, add_to=False), _aid(1024, 1, 1, 0.1),
    _aid(1025, 6, 1, 0.1), _aid(2500, 17, 1, 1.0), _aid(2500, 1, 0, 0.5),
])


def actinv_det_inputs(case):
    g = _gen(case)
    n, A = case["n"], case["A"]
    ld_o, ld_a, _ = bc_strides(case, A)
    out_a = (torch.rand(n, A, generator=g) * 2.0 - 1.0) * DET_OUT_MAX
    out_o = (torch.rand(n, A, generator=g) * 2.0 - 1.0) * DET_OUT_MAX
    out_o = torch.atanh(_away_from(torch.tanh(out_a), torch.tanh(out_o)))   # (what moved lies nearer 0: |out_o| stays <= 1.5)
    return dict(out_o=_padded(out_o, ld_o), out_a=_padded(out_a, ld_a))


def actinv_det_ref(inp, case, dtype=F64):
    """learning_utils.py:272-285 with a = o_dist.sample() = loc at the original observation"""
    A = case["A"]
    oo = inp["out_o"][:, :A].to(dtype)
    oa = inp["out_a"][:, :A].to(dtype).clone().requires_grad_(True)
    a_s = torch.tanh(oo)
    olp, alp = orc.det_normal_log_prob(oo, a_s), orc.det_normal_log_prob(oa, a_s)
    loss = F.mse_loss(olp, alp)
    (case["coeff"] * loss).backward()
    return dict(d_out=oa.grad, loss=loss.detach().reshape(1), total=(PRE + case["coeff"] * loss).detach().reshape(1),
                terms=((olp - alp) ** 2).detach()[:, 0])


# ------------------------------------------------------------------------------------------------ ssac_actor_loss_bwd_adv
def _aa(n, nets, ent, popart, pop, inv):
    return dict(n=n, nets=nets, ent=ent, popart=popart, pop=pop, inv=inv, family="actor_adv")


ACTOR_ADV = _with_ids("aa", [
    _aa(1, 1, 0, None, 0, 1.0), _aa(63, 2, 1, POP_GENERAL, 1, 1.0), _aa(65, 3, 1, POP_GENERAL, 1, 0.5),
    _aa(1024, 2, 1, POP_GENERAL, 0, 1.0), _aa(1025, 5, 0, POP_GENERAL, 1, 1.0), _aa(2500, 3, 1, None, 0, 0.5),
])
LOG_ALPHA = math.log(0.2)


def actor_adv_inputs(case):
    g = _gen(case)
    n = case["n"]
    # adv is drawn on its own: it differs from w min Q + b, so a log built from Q instead of adv misses
    return dict(q=_randn(g, case["nets"], n), logp=_randn(g, n) * 2.0 - 3.0, adv=_randn(g, n),
                log_alpha=torch.tensor([LOG_ALPHA]))


def actor_adv_ref(inp, case, dtype=F64):
    """learning.py:392-408 with use_baseline: vals = A(s, a_theta) = Q'(s, a_theta) - V(s); only Q' carries a gradient"""
    q = inp["q"].to(dtype).clone().requires_grad_(True)
    qp = q.min(0).values
    if case["popart"] and case["pop"]:
        qp = case["popart"][0] * qp + case["popart"][1]
    vals = inp["adv"].to(dtype) + (qp - qp.detach())
    bonus = inp["log_alpha"].to(dtype).exp() * inp["logp"].to(dtype) if case["ent"] else torch.zeros_like(vals)
    loss = -(vals - bonus).mean() * case["inv"]
    loss.backward()
    route = torch.zeros_like(q, dtype=torch.bool)
    route[q.detach().argmin(0), torch.arange(case["n"])] = True
    return dict(dq=q.grad, route=route, logs=(PRE + loss).detach().reshape(1), terms=((vals - bonus) * case["inv"]).detach())


# ------------------------------------------------------------------------------------------------ ssac_dr3_add
DR3_GRID = 256 * 256   # the launch: 256 workgroups of 256 threads, grid-stride
DR3 = _with_ids("dr3", [dict(N=1, B=5, H=7, family="dr3"), dict(N=2, B=128, H=256, family="dr3"),
                        dict(N=2, B=130, H=257, family="dr3")])
DR3_COEF = 0.37


def dr3_inputs(case):
    g = _gen(case)
    shape = (case["N"], 2 * case["B"], case["H"])
    z = _randn(g, *shape)
    return dict(z=z, h2=F.relu(z), dz2=_randn(g, *shape))   # h2: a ReLU output, about half exact zeros


def dr3_ref(inp, case, dtype=F64):
    """learning.py:100-108, differentiated through the ReLU that made h2"""
    B = case["B"]
    z = inp["z"].to(dtype).clone().requires_grad_(True)
    h = F.relu(z)
    prod = h[:, :B] * h[:, B:]
    (DR3_COEF * prod.sum()).backward()
    rows = prod.detach().sum(-1)
    return dict(dz2=inp["dz2"].to(dtype) + z.grad, dot=rows.mean().reshape(1), terms=prod.detach().abs().sum(-1))


# ------------------------------------------------------------------------------------------------ backup weights
def _w(kind, n, E, temp):
    return dict(n=n, E=E, temp=temp, family=f"{kind}_t{int(temp)}")


SOFTMAX = _with_ids("smw", [
    _w("softmax", 1, 2, 1.0), _w("softmax", 1, 5, 2000.0), _w("softmax", 63, 5, 20.0), _w("softmax", 65, 2, 2000.0),
    _w("softmax", 1023, 5, 1.0), _w("softmax", 1024, 2, 20.0), _w("softmax", 1025, 5, 2000.0), _w("softmax", 2500, 5, 20.0),
    _w("softmax", 2500, 2, 1.0), _w("softmax", 65, 5, 1.0),
])
SUNRISE = _with_ids("srw", [
    _w("sunrise", 1, 2, 20.0), _w("sunrise", 65, 5, 20.0), _w("sunrise", 1023, 2, 20.0), _w("sunrise", 1024, 2, 20.0),
    _w("sunrise", 1025, 5, 20.0), _w("sunrise", 2500, 5, 20.0),
])


def weights_inputs(case):
    """sunrise: members that nearly agree (std ~ 0.05), or sigmoid(-20 std) is 0 and every weight the same 0.5"""
    return dict(q=_randn(_gen(case), case["E"], case["n"]) * (0.05 if case["family"].startswith("sunrise") else 1.0))


def _std0(q):
    """q.std(0) (unbiased), spelled out: torch's CPU std accumulates float32 input in double, which would make the float32
    evaluation of these references better than any float32 kernel can be"""
    d = q - q.sum(0) / q.shape[0]
    return ((d * d).sum(0) / (q.shape[0] - 1)).sqrt()


def _weight_logs(w):
    std = w.std() if w.numel() > 1 else torch.zeros((), dtype=w.dtype)   # (one row: the kernels log 0)
    return torch.stack((w.mean(), w.max(), w.min(), std))


def softmax_weights_ref(inp, case, dtype=F64):
    """learning_utils.py:383-393"""
    w = case["n"] * F.softmax(-_std0(inp["q"].to(dtype)) * case["temp"], dim=0)
    return dict(w=w, logs=_weight_logs(w), terms=w)


def sunrise_weights_ref(inp, case, dtype=F64):
    """learning_utils.py:372-382"""
    w = torch.sigmoid(-_std0(inp["q"].to(dtype)) * case["temp"]) + 0.5
    return dict(w=w, logs=_weight_logs(w), terms=w)


# ------------------------------------------------------------------------------------------------ ssac_ensemble_min_select
def _ms(n, nets, qd, act, ld=0):
    return dict(n=n, nets=nets, qd=qd, act=int(act), ld=ld)


MIN_SELECT = _with_ids("ms", [
    _ms(1, 1, 1, False), _ms(65, 3, 4, False), _ms(1025, 2, 1, False), _ms(2500, 2, 4, False),
    _ms(1, 1, 4, True, 1), _ms(65, 2, 4, True, 1), _ms(1025, 3, 4, True, 2), _ms(2500, 2, 4, True, 2),
    _ms(65, 2, 1, True, 1), _ms(1025, 3, 1, True, 1),
    _ms(70000, 2, 4, False),   # 280 000 outputs: past the 1024 x 256 grid, the second grid-stride trip
])


def min_select_inputs(case):
    g = _gen(case)
    idx = torch.randint(0, case["qd"], (case["n"],), generator=g)
    return dict(q=_randn(g, case["nets"], case["n"], case["qd"]), idx=idx,
                act=_index_column(idx, case["ld"], case["qd"]) if case["act"] else None)


def min_select_ref(inp, case, dtype=F64):
    """agent.py:37-38, then .gather(-1, a.long()) (learning_utils.py:375, 389)"""
    m = inp["q"].to(dtype).min(0).values
    return dict(out=m.gather(-1, inp["idx"][:, None])[:, 0] if case["act"] else m)


# ------------------------------------------------------------------------------------------------ the registry
# kernel -> (cases, inputs, reference, outputs compared per element against rtol(family))
KERNELS = {
    "adv_filter": (ADV_FILTER, adv_filter_inputs, adv_filter_ref, ("adv", "prio")),
    "adv_filter_discrete": (ADV_FILTER_DISCRETE, adv_filter_discrete_inputs, adv_filter_discrete_ref, ("adv", "prio")),
    "bc_logprob": (BC_LOGPROB, bc_logprob_inputs, bc_logprob_ref, ("d_out",)),
    "bc_discrete": (BC_DISCRETE, bc_discrete_inputs, bc_discrete_ref, ("d_out",)),
    "bc_det": (BC_DET, bc_det_inputs, bc_det_ref, ("d_out",)),
    "actinv_det": (ACTINV_DET, actinv_det_inputs, actinv_det_ref, ("d_out",)),
    "actor_adv": (ACTOR_ADV, actor_adv_inputs, actor_adv_ref, ("dq",)),
    "dr3": (DR3, dr3_inputs, dr3_ref, ("dz2",)),
    "softmax": (SOFTMAX, weights_inputs, softmax_weights_ref, ("w",)),
    "sunrise": (SUNRISE, weights_inputs, sunrise_weights_ref, ("w",)),
    "min_select": (MIN_SELECT, min_select_inputs, min_select_ref, ()),
}
_CACHE = {}


def ids(kernel):
    return [c["id"] for c in KERNELS[kernel][0]]


def load(kernel, case_id):
    """(case, inputs, float64 reference): drawn and evaluated once, shared by every test that asks; treat as read-only"""
    if case_id not in _CACHE:
        cases, make, ref, _ = KERNELS[kernel]
        case = next(c for c in cases if c["id"] == case_id)
        inp = make(case)
        _CACHE[case_id] = (case, inp, ref(inp, case, F64))
    return _CACHE[case_id]
