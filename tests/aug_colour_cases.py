"""Cases of the colour-augmentation fixtures (tests/golden/aug_jitter_*, aug_netrand_*, aug_colour_*.npz), shared by
tools/gen_aug_colour_golden.py (which runs the reference) and the tests (which replay the recorded draws through
super_sac_amd.rng).  Helpers only; no tests here.

A case is a sequence of (class name, constructor kwargs) applied to a seeded uint8-valued image batch of B x c x h x w
(h != w allowed).  A fixture records, per batch k (s and s' of one AugmentationSequence call): the input ``in{k}``, the
reference's fp32 output ``out{k}`` and, for every ColorJitterAug member, the contrast-first flags of its frame groups
``order{k}`` (members x groups) -- they are drawn per application.  The parameters of member j are ``p{j}_{attribute}``.
``ref_dev64`` is the largest distance, on the 0..255 scale, of a reference output from the fp64 restatement below
(``restate``), which is written from the formulas (include/ssac_hip.h: ssac_aug_colour_jitter, ssac_aug_netrand), not from
the reference's code.  Kernel outputs are compared with the RESTATEMENT, within TOL_FACTOR x ref_dev64, every element.
"""
import os

import numpy as np
import torch

import aug_cases

GOLDEN = aug_cases.GOLDEN
TOL_FACTOR = 4.0   # the kernel is fp32 like the reference and may differ from it by its reduction order, FMA contraction and
#                    its division / remainder sequence: each one more rounding of the size the reference already makes

JITTER_FACTORS = ("factor_contrast", "factor_hue", "factor_brightness", "factor_saturate")
STATE = dict(aug_cases.STATE, ColorJitterAug=JITTER_FACTORS, NetworkRandomizationAug=("conv",))
HOOK = dict(aug_cases.HOOK, ColorJitterAug="draw_color_jitter", NetworkRandomizationAug="draw_netrand_conv")

_J, _N = ("ColorJitterAug", {}), ("NetworkRandomizationAug", {})
CASES = {
    # the seed is searched until s and s' get different orders
    "aug_jitter_c3": dict(members=[_J], B=4, c=3, h=20, w=20, both=True, base_seed=501),
    # both orders among the three groups; 1296 pixels make the strided sweeps loop
    "aug_jitter_c9": dict(members=[_J], B=3, c=9, h=36, w=36, both=False, base_seed=502),
    # scalar paths, h != w, a leftover channel
    "aug_jitter_odd": dict(members=[_J], B=3, c=7, h=17, w=19, both=False, base_seed=503),
    "aug_netrand_c3": dict(members=[_N], B=4, c=3, h=20, w=20, both=True, base_seed=504),
    "aug_netrand_odd": dict(members=[_N], B=3, c=7, h=17, w=19, both=False, base_seed=505),
    # three passes; jitter reads a float temporary
    "aug_colour_mixed": dict(members=[("TranslateAug", {}), _J, ("HorizontalFlipAug", {})], B=4, c=6, h=24, w=24, both=False,
                             base_seed=506),
    "aug_netrand_mixed": dict(members=[("CutoutAug", dict(pivot_h=4, pivot_w=6)), _N, ("VerticalFlipAug", {})], B=4, c=3,
                              h=32, w=32, both=False, base_seed=507),
}
JITTER_CASES = tuple(n for n, s in CASES.items() if any(cls == "ColorJitterAug" for cls, _ in s["members"]))

# the reference's learning_utils.sample_move_and_augment on a reference ReplayBuffer of uint8 frames: gather through idx, the
# mix, the draw order of a whole call
SMAA = dict(name="aug_colour_smaa", members=[_J, ("TranslateAug", {})], B=8, c=3, h=24, w=24, rows=24, act=2,
            mixes=(0.0, 0.5, 1.0), seed=508)

# blocks planted into every group of three channels of a jitter image: (r, g, b), 2 x 2 pixels each, side by side from (1, 1)
PLANTED = {"grey": (100, 100, 100), "black": (0, 0, 0), "r_eq_g": (200, 200, 50), "g_eq_b": (40, 180, 180),
           "white": (255, 255, 255), "primary": (255, 0, 0)}


def images(seed, B, c, h, w, planted=True):
    """seeded uint8 noise; with `planted`, every group of three channels of every row carries the PLANTED blocks"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (B, c, h, w)).astype(np.uint8)
    if planted:
        for g in range(c // 3):
            for k, rgb in enumerate(PLANTED.values()):
                img[:, 3 * g:3 * g + 3, 1:3, 1 + 2 * k:3 + 2 * k] = np.array(rgb, np.uint8).reshape(1, 3, 1, 1)
    return img


def planted_present(img):
    """every PLANTED block is where `images` put it, in every group of every row"""
    B, c, h, w = img.shape
    for g in range(c // 3):
        for k, rgb in enumerate(PLANTED.values()):
            blk = img[:, 3 * g:3 * g + 3, 1:3, 1 + 2 * k:3 + 2 * k]
            if blk.shape[2:] != (2, 2) or not (blk == np.array(rgb, np.uint8).reshape(1, 3, 1, 1)).all():
                return False
    return c >= 3


def smaa_transitions(spec=SMAA):
    rs = np.random.RandomState(spec["seed"])
    n = spec["rows"]
    s = {"obs": images(spec["seed"] + 1, n, spec["c"], spec["h"], spec["w"])}
    s1 = {"obs": images(spec["seed"] + 2, n, spec["c"], spec["h"], spec["w"])}
    a = rs.uniform(-1, 1, (n, spec["act"])).astype(np.float32)
    r = rs.randn(n, 1).astype(np.float32)
    d = (rs.rand(n, 1) < 0.1)
    return s, a, r, s1, d


def build(mod, spec):
    return [getattr(mod, cls)(spec["B"], **kw) for cls, kw in spec["members"]]


def snapshot(augs, spec):
    out = {}
    for j, (aug, (cls, _)) in enumerate(zip(augs, spec["members"])):
        for attr in STATE[cls]:
            v = getattr(aug, attr)
            if attr == "conv":
                v = v.weight
            out[f"p{j}_{attr}"] = v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v).copy()
    return out


def n_groups(spec):
    return spec["c"] // 3


def _hook_value(cls, rec, j):
    if cls == "ColorJitterAug":
        return tuple(torch.from_numpy(np.array(rec[f"p{j}_{a}"])) for a in JITTER_FACTORS)
    if cls == "NetworkRandomizationAug":
        return torch.from_numpy(np.array(rec[f"p{j}_conv"]))
    return aug_cases._hook_value(cls, rec, j)


class DrawReplay:
    """replaces the rng.draw_* hooks of the case's classes so that the next `repeat` randomisations of member j return the
    recorded parameters, and rng.draw_jitter_order so that the following applications return the recorded flags in the
    order the reference consumed them: batch-major (the batches named in `batches`), member, frame group.  `calls` lists the
    (batch_size, prob) arguments draw_jitter_order was called with."""

    def __init__(self, rng_mod, spec, rec, repeat=1, batches=(0,)):
        self.rng, self.saved, self.queues, self.calls = rng_mod, {}, {}, []
        for _ in range(repeat):
            for j, (cls, _kw) in enumerate(spec["members"]):
                self.queues.setdefault(HOOK[cls], []).append(_hook_value(cls, rec, j))
        self.flags = [bool(f) for k in batches if f"order{k}" in rec for f in np.asarray(rec[f"order{k}"]).reshape(-1)]

    def _order(self, batch_size, prob):
        self.calls.append((batch_size, prob))
        return self.flags.pop(0)

    def __enter__(self):
        for hook, queue in self.queues.items():
            self.saved[hook] = getattr(self.rng, hook)
            setattr(self.rng, hook, lambda *a, _q=queue, **k: _q.pop(0))
        self.saved["draw_jitter_order"] = self.rng.draw_jitter_order
        self.rng.draw_jitter_order = self._order
        return self

    def __exit__(self, *exc):
        for hook, fn in self.saved.items():
            setattr(self.rng, hook, fn)


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def order_bits(flags):
    """the contrast_first mask of ssac_aug_colour_jitter from one member's per-group flags"""
    return sum(1 << g for g, f in enumerate(np.asarray(flags).reshape(-1)) if f)


# ------------------------------------------------------------------------------------------ the fp64 restatement
def _clip01(x):
    return np.clip(x, 0.0, 1.0)


def contrast64(rgb, fc):
    """rgb (B, 3, h, w) in 0..1, fc (B,): clamp((x - mean) * fc + mean), the mean over (h, w) per image and channel"""
    mean = rgb.mean(axis=(2, 3), keepdims=True)
    return _clip01((rgb - mean) * fc.reshape(-1, 1, 1, 1) + mean)


def hsv_block64(rgb, fh, fb, fs, eps=1e-8):
    """rgb -> hsv, brightness, hue, saturation, hsv -> rgb of (B, 3, h, w) in 0..1 with per-row factors (B,)"""
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    cmax, cmin = rgb.max(axis=1), rgb.min(axis=1)
    delta = cmax - cmin
    hue = np.zeros_like(cmax)
    # assigned for Cmax == r, then == g, then == b: on ties b wins over g over r; the floor-mod on the r branch only
    hue = np.where(cmax == r, np.mod((g - b) / (delta + eps), 6.0), hue)
    hue = np.where(cmax == g, (b - r) / (delta + eps) + 2.0, hue)
    hue = np.where(cmax == b, (r - g) / (delta + eps) + 4.0, hue)
    hue = np.where(cmax == 0, 0.0, hue) / 6.0
    sat = np.where(cmax == 0, 0.0, delta / (cmax + eps))
    val = cmax
    fh, fb, fs = (f.reshape(-1, 1, 1) for f in (fh, fb, fs))
    val = _clip01(val * fb)
    hue, sat = _clip01(hue), _clip01(sat)
    hue = np.mod(hue + fh * 255.0 / 360.0, 1.0)                     # (it really is 255 / 360)
    sat = _clip01(sat * fs)
    hue, val = _clip01(hue), _clip01(val)
    deg = hue * 360.0
    ch = val * sat
    x = -ch * (np.abs(np.mod(deg / 60.0, 2.0) - 1.0) - 1.0)
    m = val - ch
    zero = np.zeros_like(ch)
    rp, gp, bp = zero, zero, zero                                  # a hue of exactly 360 matches no sector: (m, m, m)
    for k, (lo, (sr, sg, sb)) in enumerate(zip(range(0, 360, 60), [(ch, x, zero), (x, ch, zero), (zero, ch, x),
                                                                    (zero, x, ch), (x, zero, ch), (ch, zero, x)])):
        inside = (deg >= lo) & (deg < lo + 60)
        rp, gp, bp = np.where(inside, sr, rp), np.where(inside, sg, gp), np.where(inside, sb, bp)
    return _clip01(np.stack([rp + m, gp + m, bp + m], axis=1))


def jitter64(img, factors, flags):
    """ColorJitterAug on (B, c, h, w) values of the 0..255 scale: factors = (contrast, hue, brightness, saturation), each
    (B,); flags[g] True = group g applies contrast before the HSV block.  fp64 throughout."""
    fc, fh, fb, fs = (np.asarray(f, np.float64).reshape(-1) for f in factors)
    x = np.asarray(img, np.float64) / 255.0
    out = x.copy()
    for g in range(x.shape[1] // 3):
        rgb = x[:, 3 * g:3 * g + 3]
        if flags[g]:
            rgb = hsv_block64(contrast64(rgb, fc), fh, fb, fs)
        else:
            rgb = contrast64(hsv_block64(rgb, fh, fb, fs), fc)
        out[:, 3 * g:3 * g + 3] = rgb
    return out * 255.0


def netrand64(img, weight):
    """NetworkRandomizationAug: the zero-padded 3 x 3 cross-correlation with weight [co][ci][ky][kx] of x / 255 on every group
    of three channels, times 255, no clamp"""
    wt = np.asarray(weight, np.float64).reshape(3, 3, 3, 3)
    x = np.asarray(img, np.float64) / 255.0
    B, c, h, w = x.shape
    out = x.copy()
    for g in range(c // 3):
        pad = np.zeros((B, 3, h + 2, w + 2))
        pad[:, :, 1:-1, 1:-1] = x[:, 3 * g:3 * g + 3]
        acc = np.zeros((B, 3, h, w))
        for ky in range(3):
            for kx in range(3):
                acc += np.einsum("oi,bihw->bohw", wt[:, :, ky, kx], pad[:, :, ky:ky + h, kx:kx + w])
        out[:, 3 * g:3 * g + 3] = acc
    return out * 255.0


def _chain64(cls, kw, rec, j, x):
    """the chain members the mixed cases use, on fp64 values"""
    B, c, h, w = x.shape
    out = x.copy()
    if cls == "TranslateAug":
        t, col = np.asarray(rec[f"p{j}_translation"]), np.asarray(rec[f"p{j}_random_color"], np.float64).reshape(B, 3)
        for i in range(B):
            dy, dx = int(t[i, 0]), int(t[i, 1])
            for chn in range(c):
                out[i, chn] = col[i, chn % 3]
                ys0, ys1, xs0, xs1 = max(dy, 0), min(h + dy, h), max(dx, 0), min(w + dx, w)
                if ys0 < ys1 and xs0 < xs1:
                    out[i, chn, ys0:ys1, xs0:xs1] = x[i, chn, ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx]
    elif cls in ("HorizontalFlipAug", "VerticalFlipAug"):
        sel = np.asarray(rec[f"p{j}_random_inds"], bool)
        out[sel] = x[sel][:, :, :, ::-1] if cls == "HorizontalFlipAug" else x[sel][:, :, ::-1]
    elif cls == "CutoutAug":
        ph, pw = kw.get("pivot_h", 12), kw.get("pivot_w", 24)
        for i in range(B):
            h1, w1 = int(rec[f"p{j}_h1"][i]), int(rec[f"p{j}_w1"][i])
            out[i, :, ph + h1:ph + 2 * h1, pw + w1:pw + 2 * w1] = 0.0
    else:
        raise KeyError(cls)
    return out


def restate(spec, rec, k=0, img=None):
    """the whole case in fp64: batch k of the fixture (or `img`) through every member, with the recorded parameters and
    order flags"""
    x = np.asarray(rec[f"in{k}"] if img is None else img, np.float64)
    jit = 0
    for j, (cls, kw) in enumerate(spec["members"]):
        if cls == "ColorJitterAug":
            x = jitter64(x, [rec[f"p{j}_{a}"] for a in JITTER_FACTORS], np.asarray(rec[f"order{k}"])[jit])
            jit += 1
        elif cls == "NetworkRandomizationAug":
            x = netrand64(x, rec[f"p{j}_conv"])
        else:
            x = _chain64(cls, kw, rec, j, x)
    return x
