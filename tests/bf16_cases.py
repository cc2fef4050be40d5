"""Seeded inputs, layout helpers, float64 references and the tolerance table for the bf16 critic update of csrc/ssac_bf16.hip:
ssac_bf16_wgrad_lossfold (gradient and Adam mode), ssac_bf16_polyak and the critic saves of ssac_bf16_chain_update.  Helpers only,
no tests and no GPU imports: tests/test_hip_bf16_update.py runs the kernels on these inputs, tests/test_bf16_cases_cpu.py proves the
inputs and bounds fit for purpose without a kernel.  The layout follows wgrad_cases.py (the fp32 forms).

Rounding points, read off the kernels
-------------------------------------
* f2bf is `(__bf16)x`: a float -> bfloat conversion, round to nearest even (v_cvt_pk_bf16_f32 on gfx950; test_hip_bf16.py has the
  shadows equal torch's RNE conversion bit for bit).  ``bf16_round`` is that conversion on the CPU.
* bf_mlp_body, MODE_CRITIC_U (the critic workgroups of ssac_bf16_chain_update), per 32-row tile:
    XT   = bf16(x), transposed: feature rows [0, K1P) of the batch columns [0, n_rows) are written -- the rows [in_dim, K1P) with
           the x tile's zero K-pad (NOT left alone, as the issue that asked for these tests read it); the rows from K1P to the
           buffer's 32-row rounding and every pad column keep what they held;
    H1T  = bf16(max(acc + b1, 0)),  acc = fp32 MFMA sum over K1P of bf16(x) bf16(W1), b1 the fp32 master;
    H2T  = bf16(max(acc + b2, 0)),  acc over the STORED bf16 h1 and bf16(W2);
    DZ2uT = bf16(W3)[j] (the shadow's W3, as stored) where the stored h2 is positive (bf_pos: not zero, not negative), else 0;
    DZ1uT = bf16(acc) where the stored h1 is positive, else 0,  acc = sum_j dz2u[j] bf16(W2)[j][i] read from the W2^T shadow;
    Q    = fp32 sum of the stored bf16 h2 times w3f + b3.  w3f is the WIDENED SHADOW (bf2f of the shadow's W3 row staged in LDS),
           not the fp32 master; b3 is the master.
  All acc are fp32 MFMA accumulations (v_mfma_f32_32x32x16_bf16) of exact bf16 x bf16 products.  The library is built with
  -ffp-contract=off: the VALU sums (bias, head, Adam) are separate multiplications and additions, as emulated here.
* bf_wgrad_kernel, with c_b = dL/dq of (net, row b) from loss_fold_table (fp32, the fp32 forms' arithmetic):
    dW[j][i] = sum_b bf16(fl32(c_b dz[b][j])) h[b][i]: scale_frag forms the product in fp32 and re-rounds it to bf16 for the MFMA's
               A operand; ONE wave owns an element and adds its 16-row K-steps in order (no split-K);
    db[j]    = sum_b fl32(c_b dz[b][j]), fp32, NOT re-rounded: per lane the 8 rows of its k-half step by step, the two halves
               added by one __shfl_xor(colsum, 32);
    dW3[i]   = sum_b c_b h2[b][i] as four interleaved partial sums (rows b % 32 in [8q, 8q + 8)), then (g0 + g1) + (g2 + g3);
    db3      = sum_b c_b: lane l of wave 0 takes rows l, l + 64, ..., then a butterfly over the 64 lanes.
  Rows b >= n_rows of the table are zero, so finite pad columns [n_rows, Bp) of the saves contribute nothing.
* adam_elem: g + wd p; m + (1 - beta1)(g - m); v beta2 + (1 - beta2) g g; v_sqrt_f32(v) * (1 / bc2_sqrt) + eps; p - step_size
  (m * v_rcp_f32(denom)).  The shadows are f2bf of the NEW master (and of the new target), the W2^T quad from the same values.

Input kinds of the weight-gradient launch (gradient mode; ``kinds(case)``)
---------------------------------------------------------------------------
* "grid": operands are integers in [-3, 3] (exact in bf16), Q / td / reward / log pi on the integer grid, gamma 0.5, log alpha 0,
  weights from {0.5, 1, 2}, PopArt none or POP_EXACT, denom * n_rows a power of two (``grid_ok``).  c * dz is then a multiple of
  2^-k with at most 5 significant bits: it survives the bf16 re-rounding, and every sum is exact in float32 in any order
  (n_rows <= 8192: partial sums stay below 2^24 units).  All six segments are compared BIT FOR BIT.  The CPU test evaluates every
  grid case in float32 in two K orders with the re-rounding emulated and requires the float64 bits.
* "exact" (gauss-exact-scale): standard normal operands rounded to bf16 (about a third of dz zero, non-positive h2 included), the
  planted rows below.  td is given and c_b = g w_b err_b is exactly representable with few significant bits: g = -2 pw / (denom n)
  is a power of two (for n_rows not a power of two PopArt is on with pw = n / 2^floor(log2 n), pb = 0, which cancels the division
  exactly), w_b comes from {0.5, 1, 2}, and err_b = pw (k_b - q_b) + err0_b with integers k_b, q_b (|k_b - q_b| <= 1; 0 on planted
  rows), td_b = pw k_b + err0_b and err0_b from {+-1, +-1.5} x 2^{-2..0} (planted rows: x 2^3).  For n_rows a power of two c_b
  itself comes from powers of two times a multiple of 1/8 below 4; otherwise it carries at most 13 significant bits.  Either
  way c * dz is exact in float32 (asserted), its bf16 rounding deterministic; the reference applies the same rounding.
* "general" (gauss-general): gaussian Q, td given or evaluated in-launch from ssac_td_spec, weights from U(0.5, 1.5) or none,
  PopArt per case (POP_GENERAL with pop 0 and 1).  c_b is known to the reference within ``u_c`` (the forward error of the
  kernel's formula, one rounding of 2^-24 per operation, doubled).  A term whose product c dz lies within |dz| u_c + 2^-23 |c dz|
  of a bf16 rounding boundary may round either way on the device: it is FLAGGED and adds one bf16 ulp of the product times |h| to
  its element's bound; nothing else changes.

Planted rows (exact / general): the first row, the last row, the first row of the last 16-row K-step, rows 255 and 256 hold
sign(z) * 8 * (1 + |z|) in every operand (h2: positive) and an |err| 8 times the others', so that losing any one of them moves
every output element by at least 100 x its bound (asserted on the CPU).

Bounds.  Per element |got - ref| <= C * 2^-24 * S (+ the flagged terms' ulps), S = sum_b |a_b| |b_b| for a weight (a = the re-rounded
scaled dz, or c for the head), sum_b |a_b| for a bias.  C is measured on the CPU, never on the device: the worst
|f32 - f64| / (2^-24 S) over all cases of a float32 emulation in the kernel's orders (above), c_b itself evaluated in float32 by the
kernel's formula; C = max(8, 4 x measured), recorded and asserted PER KIND.

  constant           measured   chosen   (measured: this module's cases, numpy float32 on the CPU; test_bf16_cases_cpu.py re-measures)
  C_WEIGHT exact     8.8        35.2     (fc1, fc2, head weights, float32 accumulation only: the worst is a 1000-row chain of 63 steps)
  C_BIAS   exact     3.0        12.0     (b1, b2, b3, float32 accumulation only)
  C_WEIGHT general   10.2       40.8     (as above + the float32 error of c; the worst are cases whose td - (pw q + pb) cancels)
  C_BIAS   general   10.5       42.0     (the same cases)
  C_Q        2.3        9.2      (the chain's accumulations: one sequential chain of 16-column MFMA steps per element, the head's
                                  16 lane sums and shuffle tree)

The chain's saves are checked LAYER BY LAYER (``check_critic_saves``): each stage against a float64 reference evaluated from the
device's own previous stage.  A float32 pre-activation within the band C_Q 2^-24 S of the float64 one rounds, bf16 and ReLU being
monotone, to a value in [bf16(relu(pre - band)), bf16(relu(pre + band))]: the two ends are the same bf16 number -- the stored value
must be exactly it -- except where the band reaches a rounding boundary (neighbours one bf16 ulp apart) or zero.  XT, DZ2uT and
DZ1uT's zero pattern are exact.  Under 2 % of each buffer may lie at such a boundary (CPU test, on a float32 emulation of the chain).

Adam mode runs on grid inputs (the gradient is exact).  ``adam_ref`` propagates, next to the float64 values, a first-order error
bound through adam_elem: 2^-24 |result| per IEEE operation (the subtraction 1 - beta, the division 1 / bc2_sqrt included) and
2^-23 |result| for v_sqrt_f32 and v_rcp_f32 (documented 1 ulp), each input's error carried by the operation's derivative.  The
tolerance of m, v, p and target is twice that bound plus one float32 ulp of the stored value (``adam_tol``).
ssac_bf16_polyak alone: 2^-23 (|T| + |S|) per element.  sumsq / td_out / partials: the rules of wgrad_cases.py.
"""
import math
import zlib

import numpy as np

from offline_head_cases import POP_EXACT, POP_GENERAL, SENT, TAIL
from wgrad_cases import BETA1, BETA2, EPS24, F32, F64, GAMMA_GAUSS, GAMMA_GRID, LR, PLANT, SEGS, TAU, layout, td_ref, td_tol, ulp32

MEASURED = {"exact": {"C_WEIGHT": 8.8, "C_BIAS": 3.0}, "general": {"C_WEIGHT": 10.2, "C_BIAS": 10.5}, "C_Q": 2.3}
C_GRAD = {kind: {k: max(8.0, 4.0 * v) for k, v in MEASURED[kind].items()} for kind in ("exact", "general")}
C_Q = max(8.0, 4.0 * MEASURED["C_Q"])
GAP = 3                   # sentinel words in front of and behind a net's sumsq slots
SHADOW_SENT = 0x4321      # what a shadow word holds before a launch that must (or must not) write it
PAD_ONE = 0x3F80          # bf16 1.0: the finite sentinel of the pad-column contract


# ------------------------------------------------------------------------------------------------ bf16 and the fragment layout
def bf16_bits(x):
    """float32 -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    return bf16_widen(bf16_bits(x)).reshape(np.shape(x))


def bf16_ulp(x):
    """spacing of the bf16 grid at |x| (float64; at least the smallest normal's)"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, F64)), 2.0 ** -126)))
    return 2.0 ** (e - 7.0)


def unfrag(flat, n_rows, n_cols):
    """fragment-major -> row-major: element (n, k) lives at (((n // 32) * steps + k // 16) * 64 + n % 32 +
    32 * (k // 8 % 2)) * 8 + k % 8 -- K-step t of a 32-row block is one contiguous KiB (csrc/ssac_bf16.hip, frag_off).
    Works on a torch tensor and on a numpy array; the one copy of the formula under tests/"""
    t = flat.reshape(n_rows // 32, n_cols // 16, 2, 32, 8)                  # [row block][K step][half][row in block][8 k]
    t = t.permute(0, 3, 1, 2, 4) if hasattr(t, "permute") else t.transpose(0, 3, 1, 2, 4)   # -> [block, row, step, half, k]
    return t.reshape(n_rows, n_cols)


def frag_index(rows, bp):
    """the fragment-major offset of every (n, k) of a rows x bp matrix (rows a multiple of 32, bp of 16)"""
    assert rows % 32 == 0 and bp % 16 == 0
    return unfrag(np.arange(rows * bp, dtype=np.int64), rows, bp)


def to_frag(mat, rows_alloc, bp, pad_bits=0, fill_bits=0):
    """row-major (rows x n) values (bf16-representable float32) -> fragment-major uint16 buffer of rows_alloc x bp words: columns
    [n, bp) of EVERY row hold pad_bits, rows beyond the matrix fill_bits in their first n columns"""
    rows, n = mat.shape
    full = np.full((rows_alloc, bp), fill_bits, np.uint16)
    full[:rows, :n] = bf16_bits(mat)
    assert np.array_equal(bf16_widen(full[:rows, :n]), np.asarray(mat, F32)), "operand is not bf16-representable"
    full[:, n:] = pad_bits
    buf = np.zeros(rows_alloc * bp, np.uint16)
    buf[frag_index(rows_alloc, bp).reshape(-1)] = full.reshape(-1)
    return buf


def from_frag(buf, rows_alloc, bp):
    """fragment-major buffer -> row-major (rows_alloc x bp) bit patterns (the inverse of to_frag)"""
    return unfrag(np.ascontiguousarray(buf, np.uint16), rows_alloc, bp)


def shadow_geom(in_dim, hidden, out_dim=1):
    """ssac_bf16_layout: (stride, o1, o2, o2t, o3, k1p)"""
    k1p = (in_dim + 15) // 16 * 16
    o2 = hidden * k1p
    o2t = o2 + hidden * hidden
    o3 = o2t + hidden * hidden
    return (o3 + out_dim * hidden + 7) // 8 * 8, 0, o2, o2t, o3, k1p


def shadow_of(params_net, in_dim, hidden, fill=0):
    """the shadow words of one net's fp32 master row (out_dim 1): W1 (K zero-padded), W2, W2^T fragment-major, W3 row-major"""
    stride, o1, o2, o2t, o3, k1p = shadow_geom(in_dim, hidden)
    off, _ = layout(in_dim, hidden, 1)
    p = np.asarray(params_net, F32)
    w1 = p[off[0]:off[0] + hidden * in_dim].reshape(hidden, in_dim)
    w2 = p[off[2]:off[2] + hidden * hidden].reshape(hidden, hidden)
    sh = np.full(stride, fill, np.uint16)
    sh[o1:o2] = to_frag(bf16_round(w1), hidden, k1p)
    sh[o2:o2t] = to_frag(bf16_round(w2), hidden, hidden)
    sh[o2t:o3] = to_frag(bf16_round(w2.T), hidden, hidden)
    sh[o3:o3 + hidden] = bf16_bits(p[off[4]:off[4] + hidden])
    return sh


def wgrad_tiles(case):
    t = (case["H"] + 63) // 64
    return t * t + t * ((case["in_dim"] + 63) // 64) + 1


def bp_of(n):
    return (n + 15) // 16 * 16


def xt_rows(in_dim):
    return (in_dim + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ cases
def _c(H, in_dim, n, nets=1, td="given", weight=0, popart=None, pop=1, denom=1.0, only=None):
    return dict(H=H, in_dim=in_dim, n=n, nets=nets, td=td, weight=weight, popart=popart, pop=pop, denom=denom, only=only, out=1)


def _with_ids(cases, prefix):
    for c in cases:
        pa = {None: "0", POP_EXACT: "ex", POP_GENERAL: "gen"}[c["popart"]]
        c["id"] = f"{prefix}-h{c['H']}-i{c['in_dim']}-n{c['n']}-N{c['nets']}-td{c['td']}-w{c['weight']}-pop{pa}{c['pop']}-den{c['denom']:g}"
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


# every hidden in {32, 64, 96, 256}, in_dim in {1, 16, 17, 23, 64, 65, 100}, n_rows in {1, 15, 16, 17, 100, 255, 256, 257, 272,
# 1000} (+ one 8192-row grid case), nets in {1, 3, 5}; every ragged hidden (32, 96) meets a ragged in_dim and a ragged n_rows.
# Workgroups per launch, (tiles2 + tiles1 + 1) * nets: 3, 4, 7, 9, 12, 15, 20, 21, 25, 27, 35, 63, 125 -- mostly not multiples of 8.
GRAD_CASES = _with_ids([
    _c(32, 17, 15), _c(32, 23, 17, nets=3, td="lazy", weight=1, popart=POP_GENERAL), _c(32, 1, 1, popart=POP_EXACT),
    _c(32, 65, 100, nets=5, weight=1), _c(32, 16, 16, td="lazy", weight=1, denom=2.0), _c(32, 100, 256, nets=3, popart=POP_EXACT, td="lazy"),
    _c(64, 17, 255, nets=3, popart=POP_GENERAL, pop=0), _c(64, 64, 256, weight=1, denom=2.0), _c(64, 65, 257, td="lazy"),
    _c(64, 100, 272, nets=3, weight=1, popart=POP_GENERAL, td="lazy"), _c(64, 23, 1000, nets=5, td="lazy", weight=1),
    _c(64, 16, 8192, td="lazy", weight=1, denom=2.0, popart=POP_EXACT, only="grid"), _c(64, 1, 16, nets=5, denom=4.0),
    _c(96, 23, 17, td="lazy"), _c(96, 65, 255, nets=3, weight=1, popart=POP_GENERAL), _c(96, 100, 257, popart=POP_GENERAL, pop=0, td="lazy"),
    _c(96, 17, 100, nets=5, td="lazy", weight=1), _c(96, 1, 15, weight=1), _c(96, 64, 256, nets=3, td="lazy", weight=1, popart=POP_EXACT),
    _c(96, 16, 1000), _c(96, 17, 272, nets=1, popart=POP_GENERAL, weight=1),
    _c(256, 23, 256, td="lazy", weight=1, denom=2.0), _c(256, 17, 100, nets=3, popart=POP_GENERAL, td="lazy"), _c(256, 100, 1000, weight=1),
    _c(256, 65, 16, nets=5, td="lazy"), _c(256, 16, 1, weight=1, popart=POP_EXACT),
], "g")

# Adam mode (grid inputs): (weight decay, target?, seeded moments and step 7?)
_ADAM_BASE = [_c(32, 1, 1, popart=POP_EXACT), _c(32, 17, 16, nets=3, td="lazy", weight=1, denom=2.0), _c(32, 100, 256, nets=1, popart=POP_EXACT),
              _c(64, 23, 256, nets=3, td="lazy", weight=1), _c(96, 23, 16, td="lazy"), _c(96, 65, 256, nets=3, weight=1, popart=POP_EXACT),
              _c(256, 17, 256, td="lazy", denom=2.0)]
_ADAM_MODES = ((0.0, 1, 0), (1e-2, 1, 1), (0.0, 0, 1), (1e-2, 1, 1), (1e-2, 1, 1), (0.0, 1, 0), (1e-2, 1, 1))
ADAM_CASES = [dict(c, wd=wd, target=tg, seeded=sd) for c, (wd, tg, sd) in zip(_with_ids(_ADAM_BASE, "a"), _ADAM_MODES)]
for _a in ADAM_CASES:
    _a["id"] += f"-wd{_a['wd']:g}-t{_a['target']}-s{_a['seeded']}"
POLYAK_CASES = _with_ids([_c(32, 17, 1, nets=3), _c(96, 65, 1, nets=1), _c(256, 23, 1, nets=2)], "p")
PAD_CASES = {"grid": GRAD_CASES[2]["id"], "exact": GRAD_CASES[0]["id"], "general": GRAD_CASES[13]["id"]}   # n_rows 1, 15, 17


def _pow2(x):
    return x > 0 and x == 2.0 ** round(math.log2(x))


def grid_ok(case):
    return (case["popart"] in (None, POP_EXACT) or not case["pop"]) and _pow2(case["denom"] * case["n"]) and case["n"] <= 8192


def kinds(case):
    if case["only"]:
        return (case["only"],)
    return (("grid",) if grid_ok(case) else ()) + ("exact", "general")


def planted_rows(n):
    return sorted({r for r in (0, n - 1, 16 * ((n - 1) // 16), 255, 256) if 0 <= r < n})


def popart_of(case, kind):
    """(pw, pb) in effect, or None"""
    if kind == "exact":
        n = case["n"]
        return None if _pow2(n) else (F32(n / 2.0 ** math.floor(math.log2(n))), F32(0.0))
    if case["popart"] is None or not case["pop"]:
        return None
    return F32(case["popart"][0]), F32(case["popart"][1])


def popart_struct(case, kind):
    """(pw, pb, pop flag) of the ssac_popart handed to the launch, or None: the case's state with pop 0 is still handed over"""
    if kind == "exact":
        pa = popart_of(case, kind)
        return None if pa is None else (float(pa[0]), float(pa[1]), 1)
    if case["popart"] is None:
        return None
    return float(case["popart"][0]), float(case["popart"][1]), int(case["pop"])


# ------------------------------------------------------------------------------------------------ inputs
def _rng(case, kind):
    return np.random.RandomState(zlib.crc32((case["id"] + kind).encode()) & 0x7FFFFFFF)


def _draw(g, kind, shape, positive_plant=False, zeros=0.0):
    """operand (..., n_rows, features) of bf16 values: grid integers, or normals with planted rows (a share `zeros` set to 0)"""
    if kind == "grid":
        return g.randint(-3, 4, size=shape).astype(F32)
    z = g.standard_normal(shape)
    if zeros:
        z[g.rand(*shape) < zeros] = 0.0
    for r in planted_rows(shape[-2]):
        zz = g.standard_normal(shape[:-2] + shape[-1:])
        z[..., r, :] = (1.0 if positive_plant else np.where(zz >= 0, 1.0, -1.0)) * PLANT * (1.0 + np.abs(zz))
    return bf16_round(z.astype(F32))


def make_inputs(case, kind):
    g = _rng(case, kind)
    n, i, h, nets = case["n"], case["in_dim"], case["H"], case["nets"]
    off, stride = layout(i, h, 1)
    grid = kind == "grid"
    params = np.full((nets, stride), SENT, F32)
    params[:, :off[5] + 1] = g.randint(-3, 4, size=(nets, off[5] + 1)).astype(F32) if grid else g.standard_normal((nets, off[5] + 1)).astype(F32)
    inp = dict(kind=kind, params=params)
    zk = "grid" if grid else "gauss"
    inp["X"] = _draw(g, zk, (n, i))
    inp["H1"] = _draw(g, zk, (nets, n, h), positive_plant=True, zeros=0.3)
    inp["H2"] = _draw(g, zk, (nets, n, h), positive_plant=True, zeros=0.3)
    if not grid:
        inp["H1"], inp["H2"] = np.abs(inp["H1"]), np.abs(inp["H2"])          # post-ReLU values
    inp["DZ2"] = _draw(g, zk, (nets, n, h), zeros=0.3)
    inp["DZ1"] = _draw(g, zk, (nets, n, h), zeros=0.3)
    lf = dict(gamma=F32(GAMMA_GRID if grid else GAMMA_GAUSS), log_alpha=F32(0.0 if grid else math.log(0.2)))
    pa = popart_of(case, kind)
    pw, pb = (F64(pa[0]), F64(pa[1])) if pa else (1.0, 0.0)
    lazy = case["td"] == "lazy" and kind != "exact"
    if kind == "exact":
        # one td per row serves every net: td = pw k + err0 and q_e = k + {-1, 0, 1} (planted rows: k), all exact in float32
        err0 = g.choice([1.0, -1.0, 1.5, -1.5], size=n) * 2.0 ** g.randint(-2, 1, size=n)
        dq = g.randint(-1, 2, size=(nets, n)).astype(F64)
        for r in planted_rows(n):
            err0[r] = g.choice([1.0, -1.0, 1.5, -1.5]) * 8.0
            dq[:, r] = 0.0
        k = g.randint(-2, 3, size=n).astype(F64)
        td = pw * k + err0
        q = k[None, :] + dq
        assert np.array_equal(td.astype(F32).astype(F64), td) and np.array_equal((pw * q).astype(F32).astype(F64), pw * q)
        lf["td"], lf["Q"] = td.astype(F32), q.astype(F32)
    else:
        if lazy:
            draw = (lambda s: g.randint(-3, 4, size=s).astype(F32)) if grid else (lambda s: g.standard_normal(s).astype(F32))
            lf["q_t"] = draw((2, n))
            lf["logp"] = draw((n,)) if grid else (g.standard_normal(n) * 2.0 - 3.0).astype(F32)
            lf["rew"] = draw((n,))
            lf["done"] = (g.rand(n) < 0.25).astype(F32)
            td = td_ref(lf)
        else:
            td = (g.randint(-3, 4, size=n) if grid else g.standard_normal(n)).astype(F32).astype(F64)
            lf["td"] = td.astype(F32)
        q = g.randint(-3, 4, size=(nets, n)).astype(F32) if grid else g.standard_normal((nets, n)).astype(F32)
        if not grid:
            for r in planted_rows(n):
                z = g.standard_normal(nets)
                q[:, r] = ((td[r] - pb - np.where(z >= 0, 1.0, -1.0) * PLANT * (1.0 + np.abs(z))) / pw).astype(F32)
        lf["Q"] = q
    if case["weight"]:
        lf["weight"] = g.choice(np.array([0.5, 1.0, 2.0], F32), size=n) if kind != "general" else g.uniform(0.5, 1.5, n).astype(F32)
    inp["lf"] = lf
    if kind == "general":   # a planted term must not sit on a rounding boundary (its ulp would rival the smaller planted terms)
        ls = loss_scale(case, inp)
        rows = np.zeros((1, n, 1), bool)
        rows[0, planted_rows(n), 0] = True
        for key in ("DZ1", "DZ2"):
            for _ in range(16):
                bad = scaled(ls["c"], inp[key], ls["u_c"])[2] & rows
                if not bad.any():
                    break
                inp[key][bad] = bf16_widen(bf16_bits(inp[key][bad]) + np.uint16(1))   # the next bf16 value away from zero
            assert not bad.any()
    return inp


def loss_scale(case, inp, dtype=F64):
    """c = dL/dq = -2 pw w (td - (pw q + pb)) / (denom n) of every net and row in loss_fold_table's operation order, err, the loss
    terms, td, and u_c: a bound of |c_device - c| (0 where the arithmetic is exact)"""
    lf, n, kind = inp["lf"], case["n"], inp["kind"]
    t = lambda a: np.asarray(a, dtype)
    pa = popart_of(case, kind)
    pw, pb = (t(pa[0]), t(pa[1])) if pa else (dtype(1.0), dtype(0.0))
    gscale = dtype(-2.0) * pw / (t(F32(case["denom"])) * dtype(n))
    td = td_ref(lf, dtype) if "q_t" in lf else t(lf["td"])
    w = t(lf["weight"]) if "weight" in lf else np.ones(n, dtype)
    pq = pw * t(lf["Q"])
    err = td[None, :] - (pq + pb)
    c = (gscale * w[None, :]) * err
    out = dict(c=c, err=err, werr2=(w[None, :] * err) * err, td=td)
    if dtype is F64:
        if kind == "general":
            u_td = td_tol(lf) if "q_t" in lf else 0.0
            u_err = u_td + 2.0 ** -23 * (np.abs(pq) + np.abs(pq + pb) + np.abs(err))
            out["u_c"] = np.abs(gscale * w[None, :]) * u_err + 8.0 * 2.0 ** -23 * np.abs(c)
        else:
            out["u_c"] = np.zeros_like(c)
    return out


def scaled(c, dz, u_c=None):
    """scale_frag in float64 + the two roundings: (v = fl32(c dz), s = bf16(v), flagged mask, bf16 ulp of the product)"""
    p = c[..., None] * np.asarray(dz, F64)
    v = p.astype(F32)
    s = bf16_round(v).astype(F64)
    ulp = bf16_ulp(np.maximum(np.abs(p), np.abs(s)))
    if u_c is None or not np.any(u_c):
        return v.astype(F64), s, np.zeros(p.shape, bool), ulp
    delta = np.abs(np.asarray(dz, F64)) * u_c[..., None] + 2.0 ** -23 * np.abs(p)
    lo = bf16_ulp(p)
    frac = np.abs(p) / lo
    dist = np.abs(frac - np.floor(frac) - 0.5) * lo          # distance to the nearest rounding boundary (a midpoint)
    flagged = (dist <= delta) & (p != 0.0)
    return v.astype(F64), s, flagged, ulp


def reference(case, inp):
    """{seg: (g, S, extra)} per net: float64 gradient, bound sum, and the flagged terms' allowance; also "flag_share" """
    ls = loss_scale(case, inp)
    c, u_c = ls["c"], ls["u_c"]
    out = {}
    nf = nt = 0
    X = np.asarray(inp["X"], F64)
    for l, dz, B in (("1", inp["DZ1"], None), ("2", inp["DZ2"], inp["H1"])):
        v, s, fl, ulp = scaled(c, dz, u_c)
        Bm = np.broadcast_to(X, (case["nets"],) + X.shape) if B is None else np.asarray(B, F64)
        out["w" + l] = (np.einsum("ekm,ekn->emn", s, Bm), np.einsum("ekm,ekn->emn", np.abs(s), np.abs(Bm)),
                        np.einsum("ekm,ekn->emn", fl * ulp, np.abs(Bm)))
        p = c[..., None] * np.asarray(dz, F64)
        out["b" + l] = (p.sum(1), np.abs(p).sum(1), np.zeros(p.shape[::2]))
        nf, nt = nf + int(fl.sum()), nt + int((p != 0).sum())
    H2 = np.asarray(inp["H2"], F64)
    out["w3"] = (np.einsum("ek,ekn->en", c, H2)[:, None, :], np.einsum("ek,ekn->en", np.abs(c), np.abs(H2))[:, None, :], np.zeros((case["nets"], 1, case["H"])))
    out["b3"] = (c.sum(1)[:, None], np.abs(c).sum(1)[:, None], np.zeros((case["nets"], 1)))
    out["flag_share"] = nf / max(nt, 1)
    out["loss"] = ls
    return out


def bound(kind, seg, S, extra=0.0):
    return C_GRAD[kind]["C_WEIGHT" if seg[0] == "w" else "C_BIAS"] * EPS24 * S + extra


def planted_terms(case, inp, ref):
    """per planted row and segment the |term| that row contributes to every element: {seg: (rows, nets, ...segment shape)}"""
    c = ref["loss"]["c"]
    rows = planted_rows(case["n"])
    out = {}
    X = np.asarray(inp["X"], F64)
    for l, dz, B in (("1", inp["DZ1"], None), ("2", inp["DZ2"], inp["H1"])):
        _, s, _, _ = scaled(c, dz, None)
        p = c[..., None] * np.asarray(dz, F64)
        out["w" + l] = np.stack([np.abs(s[:, r, :, None] * (X[r][None, None, :] if B is None else np.asarray(B, F64)[:, r, None, :])) for r in rows])
        out["b" + l] = np.stack([np.abs(p[:, r, :]) for r in rows])
    out["w3"] = np.stack([np.abs(c[:, r, None] * np.asarray(inp["H2"], F64)[:, r, :])[:, None, :] for r in rows])
    out["b3"] = np.stack([np.abs(c[:, r])[:, None] for r in rows])
    return out


# ------------------------------------------------------------------------------------------------ float32 emulation
def emul_steps(A, B):
    """A^T B in float32 as bf_wgrad_kernel adds it: one chain of 16-row K-steps per element"""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    W = np.zeros((A.shape[1], B.shape[1]), F32)
    for r in range(0, A.shape[0], 16):
        W = W + A[r:r + 16].T @ B[r:r + 16]
    return W


def emul_steps_rev(A, B):
    """another K order (last step first, rows of a step reversed): exact sums must not care"""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    W = np.zeros((A.shape[1], B.shape[1]), F32)
    for r in reversed(range(0, A.shape[0], 16)):
        W = W + A[r:r + 16][::-1].T @ B[r:r + 16][::-1]
    return W


def emul_colsum(V):
    """the bias: per k-half (rows b % 16 < 8, >= 8) one chain in row order, the halves added"""
    V = np.asarray(V, F32)
    half = [np.zeros(V.shape[1], F32), np.zeros(V.shape[1], F32)]
    for b in range(V.shape[0]):
        half[(b >> 3) & 1] = half[(b >> 3) & 1] + V[b]
    return half[0] + half[1]


def emul_head(c, H2):
    """dW3: four interleaved 8-row partial sums, (g0 + g1) + (g2 + g3); db3: 64 strided lane sums, then a butterfly"""
    c, H2 = np.asarray(c, F32), np.asarray(H2, F32)
    gq = [np.zeros(H2.shape[1], F32) for _ in range(4)]
    for b in range(c.shape[0]):
        gq[(b >> 3) & 3] = gq[(b >> 3) & 3] + c[b] * H2[b]
    lanes = np.zeros(64, F32)
    for b in range(c.shape[0]):
        lanes[b & 63] = lanes[b & 63] + c[b]
    o = 32
    while o:
        lanes = lanes + lanes[np.arange(64) ^ o]
        o >>= 1
    return (gq[0] + gq[1]) + (gq[2] + gq[3]), lanes[0]


def emulate(case, inp, order=emul_steps):
    """{seg: float32 gradient per net} by the kernel's arithmetic: c in float32 by loss_fold_table's formula, products re-rounded"""
    c = loss_scale(case, inp, F32)["c"].astype(F32)
    out = {s: [] for s in SEGS}
    for e in range(case["nets"]):
        for l, dz, B in (("1", inp["DZ1"][e], inp["X"]), ("2", inp["DZ2"][e], inp["H1"][e])):
            v = (c[e][:, None] * np.asarray(dz, F32)).astype(F32)
            out["w" + l].append(order(bf16_round(v), B))
            out["b" + l].append(emul_colsum(v) if order is emul_steps else v[::-1].sum(0, dtype=F32))
        gw, gb = emul_head(c[e], inp["H2"][e]) if order is emul_steps else ((c[e][::-1, None] * inp["H2"][e][::-1]).sum(0, dtype=F32), c[e][::-1].sum(dtype=F32))
        out["w3"].append(gw[None, :])
        out["b3"].append(np.array([gb], F32))
    return {s: np.stack(v_) for s, v_ in out.items()}


# ------------------------------------------------------------------------------------------------ Adam in float64 with its bound
def adam_state(case, shape):
    """(m, v, target) before the step: zeros, or seeded; the target always seeded"""
    g = _rng(case, "adam")
    m = (g.standard_normal(shape) * 0.5).astype(F32) if case["seeded"] else np.zeros(shape, F32)
    v = (g.uniform(0.1, 2.0, shape)).astype(F32) if case["seeded"] else np.zeros(shape, F32)
    return m, v, g.standard_normal(shape).astype(F32)


def adam_ref(ctl, p, g, m, v, target, tau=TAU):
    """adam_elem (+ Polyak on the new parameter) in float64, and per output the first-order error bound of the float32 / approximate
    evaluation (module docstring): {k: (value, error)}"""
    t = lambda a: np.asarray(a, F64)
    p, g, m, v = t(p), t(g), t(m), t(v)
    u, ua = EPS24, 2.0 ** -23
    b1, b2, wd, eps, ss = (float(ctl[k]) for k in ("beta1", "beta2", "wd", "eps", "step_size"))
    e_g = np.zeros_like(g)
    if wd != 0.0:
        g2 = g + wd * p
        e_g = u * (np.abs(wd * p) + np.abs(g2))
        g = g2
    d = g - m
    e_d = e_g + u * np.abs(d)
    t1 = (1.0 - b1) * d
    e_t1 = (1.0 - b1) * e_d + 2.0 * u * np.abs(t1)                     # (1 - beta1 rounded, the product rounded)
    mn = m + t1
    e_m = e_t1 + u * np.abs(mn)
    x1, x2 = v * b2, (1.0 - b2) * g * g
    e_x2 = 3.0 * u * np.abs(x2) + (1.0 - b2) * 2.0 * np.abs(g) * e_g   # (1 - beta2, two products)
    vn = x1 + x2
    e_v = u * np.abs(x1) + e_x2 + u * np.abs(vn)
    s = np.sqrt(vn)
    e_s = np.where(vn > 0, e_v / (2.0 * np.maximum(s, 1e-300)), np.sqrt(e_v)) + ua * s
    inv = 1.0 / float(ctl["bc2_sqrt"])
    si = s * inv
    e_si = e_s * inv + 2.0 * u * np.abs(si)                            # (the division 1 / bc2_sqrt, the product)
    den = si + eps
    e_den = e_si + u * den
    r = 1.0 / den
    e_r = e_den * r * r + ua * r
    q = mn * r
    e_q = e_m * r + np.abs(mn) * e_r + u * np.abs(q)
    st = ss * q
    e_st = ss * e_q + u * np.abs(st)
    pn = p - st
    e_p = e_st + u * np.abs(pn)
    out = dict(m=(mn, e_m), v=(vn, e_v), p=(pn, e_p))
    if target is not None:
        a, b = t(target) * (1.0 - tau), pn * tau
        tn = a + b
        out["target"] = (tn, 2.0 * u * np.abs(a) + u * np.abs(b) + tau * e_p + u * np.abs(tn))
    return out


def adam_tol(val, err):
    return 2.0 * err + ulp32(val)


def polyak_tol(T, S):
    return 2.0 ** -23 * (np.abs(np.asarray(T, F64)) + np.abs(np.asarray(S, F64)))


# ------------------------------------------------------------------------------------------------ the chained launch
LOG_STD_LO, LOG_STD_HI = -5.0, 2.0
FWD_RTOL, FWD_ATOL = 4e-3, 1e-4      # test_hip_bf16.py's stated forward tolerance: 4e-3 * max |ref| + 1e-4


def _cc(H, S, A, n, critics, n_sel, ld_pad):
    return dict(H=H, S=S, A=A, in_dim=S + A, n=n, nets=critics, n_sel=n_sel, ld_pad=ld_pad, n_targets=3, out=1,
                id=f"c-h{H}-i{S + A}-n{n}-N{critics}-sel{n_sel}-ld{ld_pad}")


# hidden {32, 96, 256} x critic in_dim {17, 23, 65} x n_rows {1, 31, 33, 100, 512} x critics {1, 3} x n_sel {1, 2} x ldxc = / > in_dim
CHAIN_CASES = [_cc(32, 11, 6, 1, 1, 1, 0), _cc(32, 17, 6, 33, 3, 2, 3), _cc(96, 57, 8, 31, 1, 2, 1), _cc(96, 11, 6, 100, 3, 1, 0),
               _cc(256, 17, 6, 512, 3, 2, 5), _cc(256, 57, 8, 100, 1, 1, 0)]
CLOSING_CASE = CHAIN_CASES[3]["id"]


def _arena(g, nets, in_dim, hidden, out_dim):
    off, stride = layout(in_dim, hidden, out_dim)
    P = np.full((nets, stride), SENT, F32)
    for j, (sz, scale) in enumerate(((hidden * in_dim, in_dim ** -0.5), (hidden, 0.05), (hidden * hidden, hidden ** -0.5), (hidden, 0.05),
                                     (out_dim * hidden, hidden ** -0.5), (out_dim, 0.05))):
        P[:, off[j]:off[j] + sz] = (g.standard_normal((nets, sz)) * scale).astype(F32)
    return P


def chain_inputs(case):
    g = _rng(case, "chain")
    S, A, H, n = case["S"], case["A"], case["H"], case["n"]
    ld = S + A + case["ld_pad"]
    Xc = np.full((n, ld), SENT, F32)
    Xc[:, :S + A] = g.standard_normal((n, S + A))
    Xc[:: 7, 0] = 0.0
    return dict(actor=_arena(g, 1, S, H, 2 * A), targets=_arena(g, case["n_targets"], S + A, H, 1), critics=_arena(g, case["nets"], S + A, H, 1),
                Xa=g.standard_normal((n, S)).astype(F32), eps=g.standard_normal((n, A)).astype(F32), Xc=Xc, ldxc=ld,
                ids=[2, 0][:case["n_sel"]] if case["n_sel"] == 2 else [1])


def net_parts(P, in_dim, hidden, out_dim):
    """(bf16 W1, b1, bf16 W2, b2, bf16 W3, b3) of one net's master row, float64: what the shadow and the kernel's bias reads hold"""
    off, _ = layout(in_dim, hidden, out_dim)
    w = lambda j, shp: np.asarray(P[off[j]:off[j] + int(np.prod(shp))], F32).reshape(shp)
    return (bf16_round(w(0, (hidden, in_dim))).astype(F64), w(1, (hidden,)).astype(F64), bf16_round(w(2, (hidden, hidden))).astype(F64),
            w(3, (hidden,)).astype(F64), bf16_round(w(4, (out_dim, hidden))).astype(F64), w(5, (out_dim,)).astype(F64))


def forward_emulation(P, in_dim, hidden, out_dim, x):
    """test_hip_bf16.py's _emulate: bf16 weights / inputs / hidden activations, float64 accumulation"""
    W1, b1, W2, b2, W3, b3 = net_parts(P, in_dim, hidden, out_dim)
    h1 = bf16_round(np.maximum(bf16_round(np.asarray(x, F32)).astype(F64) @ W1.T + b1, 0.0).astype(F32)).astype(F64)
    h2 = bf16_round(np.maximum(h1 @ W2.T + b2, 0.0).astype(F32)).astype(F64)
    return h2 @ W3.T + b3


def sample_reference(case, inp):
    """a', log pi and their tolerances from the actor's forward emulation at the forward test's tolerance"""
    A = case["A"]
    y = forward_emulation(inp["actor"][0], case["S"], case["H"], 2 * A, inp["Xa"])
    ty = FWD_RTOL * float(np.abs(y).max()) + FWD_ATOL
    mu, raw, eps = y[:, :A], y[:, A:], inp["eps"].astype(F64)
    half = 0.5 * (LOG_STD_HI - LOG_STD_LO)
    log_std = LOG_STD_LO + half * (np.tanh(raw) + 1.0)
    sd = np.exp(log_std)
    u = mu + sd * eps
    sp = np.logaddexp(0.0, -2.0 * u)
    lp = ((-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)) - 2.0 * (math.log(2.0) - u - sp)).sum(1)
    du = ty * (1.0 + np.abs(eps) * sd * half)
    return dict(a=np.tanh(u), a_tol=du + 1e-5, logp=lp, logp_tol=(ty * half + 2.0 * du).sum(1) + 1e-4)


def _interval(pre, band, relu):
    """the bf16 values a float32 pre-activation within `band` of `pre` can round to: (lo, hi), monotone in the pre-activation"""
    lo, hi = pre - band, pre + band
    if relu:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    return bf16_round(lo.astype(F32)).astype(F64), bf16_round(hi.astype(F32)).astype(F64)


def _stage(name, got_bits, pre, S, relu, mask=None):
    """a rounded stage against its float64 pre-rounding value: the stored value must be the reference's bf16 value; where the
    accumulation band C_Q 2^-24 S around `pre` reaches a bf16 rounding boundary (or zero) it may be either neighbour, nothing else.
    mask (DZ1uT): False = the element must be exactly zero.  Returns the flagged share"""
    band = C_Q * EPS24 * S
    lo, hi = _interval(pre, band, relu)
    got = bf16_widen(got_bits).astype(F64).reshape(pre.shape)
    if mask is not None:
        zero = ~mask
        assert not (got_bits.reshape(pre.shape)[zero] & 0x7FFF).any(), f"{name}: {int(((got_bits.reshape(pre.shape)[zero] & 0x7FFF) != 0).sum())} elements behind a non-positive h1 are not zero"
        lo, hi, got = lo[mask], hi[mask], got[mask]
    bad = (got < lo) | (got > hi)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements are not the reference's bf16 value (nor, inside the accumulation band of a rounding boundary, its neighbour)"
    return float((lo != hi).mean()) if lo.size else 0.0


def check_critic_saves(case, inp, dev):
    """the layered check of the critic workgroups' saves.  dev: XT (xt_rows x bp), H1T / H2T / DZ2T / DZ1T (nets x H x bp) row-major
    bit patterns as from_frag returns them, Q (nets x n) float32.  Every stage is checked against a float64 reference evaluated FROM
    THE DEVICE'S OWN PREVIOUS STAGE; returns the flagged share per buffer"""
    n, i, H = case["n"], case["in_dim"], case["H"]
    k1p = (i + 15) // 16 * 16
    x_bits = bf16_bits(inp["Xc"][:, :i]).T
    assert np.array_equal(dev["XT"][:i, :n], x_bits), f"XT: {int((dev['XT'][:i, :n] != x_bits).sum())} words differ from bf16(x) transposed"
    assert not dev["XT"][i:k1p, :n].any(), "XT: the K-pad feature rows [in_dim, K1P) of the tile are not zero"
    x = bf16_widen(dev["XT"][:i, :n]).astype(F64).T
    share = {}
    for e in range(case["nets"]):
        W1, b1, W2, b2, W3, b3 = net_parts(inp["critics"][e], i, H, 1)
        w3 = W3[0]
        h1b, h2b = dev["H1T"][e][:, :n].T, dev["H2T"][e][:, :n].T
        f = lambda k, v: share.__setitem__(k, max(share.get(k, 0.0), v))
        f("H1T", _stage(f"H1T of net {e}", h1b, x @ W1.T + b1, np.abs(x) @ np.abs(W1).T + np.abs(b1), True))
        h1 = bf16_widen(h1b).astype(F64)
        f("H2T", _stage(f"H2T of net {e}", h2b, h1 @ W2.T + b2, np.abs(h1) @ np.abs(W2).T + np.abs(b2), True))
        h2 = bf16_widen(h2b).astype(F64)
        pos2 = ((h2b & 0x7FFF) != 0) & ((h2b & 0x8000) == 0)
        dz2b = np.where(pos2, bf16_bits(w3.astype(F32))[None, :], np.uint16(0))
        assert np.array_equal(dev["DZ2T"][e][:, :n].T, dz2b), f"DZ2uT of net {e}: {int((dev['DZ2T'][e][:, :n].T != dz2b).sum())} words differ from bf16(W3) masked by the device's h2 > 0"
        dz2 = bf16_widen(dz2b).astype(F64)
        pos1 = ((h1b & 0x7FFF) != 0) & ((h1b & 0x8000) == 0)
        f("DZ1T", _stage(f"DZ1uT of net {e}", dev["DZ1T"][e][:, :n].T, dz2 @ W2, np.abs(dz2) @ np.abs(W2), False, mask=pos1))
        q, Sq = h2 @ w3 + b3[0], np.abs(h2) @ np.abs(w3) + abs(b3[0])
        bad = np.abs(dev["Q"][e].astype(F64) - q) > C_Q * EPS24 * Sq
        assert not bad.any(), f"Q of net {e}: {int(bad.sum())} rows beyond C_Q 2^-24 S, worst {float((np.abs(dev['Q'][e] - q) / (C_Q * EPS24 * Sq)).max()):.3g} bounds"
    return share


def _chain32(A, W):
    """A W^T in float32 as the MFMA chain adds it: 16 columns of K per step, one chain per element"""
    A, W = np.asarray(A, F32), np.asarray(W, F32)
    acc = np.zeros((A.shape[0], W.shape[0]), F32)
    for k in range(0, A.shape[1], 16):
        acc = acc + A[:, k:k + 16] @ W[:, k:k + 16].T
    return acc


def emulate_critic_saves(case, inp):
    """the critic workgroups' arithmetic in float32 on the CPU: `dev` as check_critic_saves takes it, and the worst
    |float32 - float64| / (2^-24 S) of every accumulation (the measurement behind C_Q)"""
    n, i, H, nets = case["n"], case["in_dim"], case["H"], case["nets"]
    bp, worst = bp_of(n), 0.0
    x = bf16_round(inp["Xc"][:, :i])
    dev = dict(XT=np.zeros((xt_rows(i), bp), np.uint16), Q=np.zeros((nets, n), F32))
    dev["XT"][:i, :n] = bf16_bits(x).T
    for k in ("H1T", "H2T", "DZ2T", "DZ1T"):
        dev[k] = np.zeros((nets, H, bp), np.uint16)

    def meas(a32, A, W, bias):
        nonlocal worst
        A, W = np.asarray(A, F64), np.asarray(W, F64)
        S = np.abs(A) @ np.abs(W).T + np.abs(bias)
        worst = max(worst, float((np.abs(a32.astype(F64) - (A @ W.T + bias)) / np.maximum(EPS24 * S, 1e-300)).max()))
    for e in range(nets):
        W1, b1, W2, b2, W3, b3 = (a.astype(F32) for a in net_parts(inp["critics"][e], i, H, 1))
        p1 = _chain32(x, W1) + b1
        meas(p1, x, W1, b1)
        h1 = bf16_round(np.maximum(p1, F32(0.0)))
        p2 = _chain32(h1, W2) + b2
        meas(p2, h1, W2, b2)
        h2 = bf16_round(np.maximum(p2, F32(0.0)))
        dz2 = np.where(h2 > 0, W3[0][None, :], F32(0.0)).astype(F32)
        p3 = _chain32(dz2, W2.T.copy())
        meas(p3, dz2, W2.T, 0.0)
        dz1 = np.where(h1 > 0, bf16_round(p3), F32(0.0)).astype(F32)
        # the head: lane xl of a row's 16 takes k in [8 xl, 8 xl + 8) + 128 m in order, then a shuffle tree over 8, 4, 2, 1
        lanes = np.zeros((n, 16), F32)
        for k0 in range(0, H, 128):
            for xl in range(16):
                for u in range(8):
                    k = k0 + 8 * xl + u
                    if k < H:
                        lanes[:, xl] = lanes[:, xl] + h2[:, k] * W3[0, k]
        o = 8
        while o:
            lanes = lanes + lanes[:, np.arange(16) ^ o]
            o >>= 1
        q = lanes[:, 0] + b3[0]
        meas(q[:, None], h2, W3, b3[0])
        dev["Q"][e] = q
        for k, a in (("H1T", h1), ("H2T", h2), ("DZ2T", dz2), ("DZ1T", dz1)):
            dev[k][e][:, :n] = bf16_bits(a).T
    return dev, worst


# ------------------------------------------------------------------------------------------------ the registry
_ALL = {c["id"]: c for c in GRAD_CASES + ADAM_CASES + POLYAK_CASES + CHAIN_CASES}
_CACHE = {}


def ids(cases):
    return [c["id"] for c in cases]


def load(case_id, kind):
    """(case, inputs, float64 reference): drawn and evaluated once, shared by every test that asks; treat as read-only"""
    key = (case_id, kind)
    if key not in _CACHE:
        case = _ALL[case_id]
        inp = make_inputs(case, kind)
        _CACHE[key] = (case, inp, reference(case, inp))
    return _CACHE[key]
