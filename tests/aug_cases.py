"""Cases of the chained-augmentation fixtures (tests/golden/aug_*.npz), shared by tools/gen_aug_golden.py (which runs the
reference) and the tests (which replay the recorded draws through super_sac_amd.rng).  Helpers only; no tests here.

A case is a sequence of (class name, constructor kwargs) applied to a seeded uint8-valued image batch.  The recorded
parameters of member j are stored as ``p{j}_{attribute}``.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# attributes that hold the randomisation of each class
STATE = {
    "CutoutAug": ("w1", "h1"), "CutoutColorAug": ("w1", "h1", "rand_box"),
    "TranslateAug": ("translation", "random_color"), "LargeTranslateAug": ("translation", "random_color"),
    "HorizontalFlipAug": ("random_inds",), "VerticalFlipAug": ("random_inds",), "RotateAug": ("random_inds",),
    "WindowAug": ("w1", "h1"), "GammaAug": ("gamma",), "Drqv2Aug": ("shift",),
}
# the rng hook that draws each class's randomisation
HOOK = {
    "CutoutAug": "draw_cutout_box", "CutoutColorAug": "draw_cutout_color", "TranslateAug": "draw_translation",
    "LargeTranslateAug": "draw_translation", "HorizontalFlipAug": "draw_flip_rows", "VerticalFlipAug": "draw_flip_rows",
    "RotateAug": "draw_rotation", "WindowAug": "draw_window", "GammaAug": "draw_gamma", "Drqv2Aug": "draw_drqv2_shift",
}
REPR = {"CutoutAug": "Cutout", "CutoutColorAug": "CutoutColor", "TranslateAug": "Translate",
        "LargeTranslateAug": "LargeTranslate", "HorizontalFlipAug": "HorizontalFlip", "VerticalFlipAug": "VerticalFlip",
        "RotateAug": "Rotate", "WindowAug": "Window", "GammaAug": "Gamma"}
CHAIN_CLASSES = tuple(REPR)

_SMALL_BOX = dict(pivot_h=4, pivot_w=6)   # (a 32 x 32 image: the default pivots would put most boxes outside)


def _single(cls, c, **over):
    big = cls in ("WindowAug", "CutoutAug", "CutoutColorAug") and c == 3   # the defaults of these want a > 64 pixel image
    hw = 76 if big else (16 if cls == "GammaAug" else 32)
    kw = dict(_SMALL_BOX) if cls in ("CutoutAug", "CutoutColorAug") and not big else {}
    spec = dict(members=[(cls, kw)], B=4 if c == 3 else 6, c=c, hw=hw, both=True, base_seed=100 + 7 * len(cls) + c)
    spec.update(over)
    return spec


SINGLES = {f"aug_{cls}_c{c}": _single(cls, c) for cls in CHAIN_CLASSES for c in (9, 3)}
CHAINS = {
    "aug_chain_tcf": dict(members=[("TranslateAug", {}), ("CutoutColorAug", dict(_SMALL_BOX)), ("HorizontalFlipAug", {})],
                          B=6, c=9, hw=32, both=True, base_seed=301),
    "aug_chain_rwgc": dict(members=[("RotateAug", {}), ("WindowAug", {}), ("GammaAug", {}), ("CutoutAug", {})],
                           B=3, c=3, hw=68, both=False, base_seed=302),
    "aug_chain_gamma2": dict(members=[("GammaAug", {}), ("VerticalFlipAug", {}), ("LargeTranslateAug", {}), ("GammaAug", {}),
                                      ("CutoutColorAug", dict(_SMALL_BOX))],
                             B=4, c=6, hw=24, both=False, base_seed=303),
    "aug_mixed_drqv2": dict(members=[("CutoutAug", dict(_SMALL_BOX)), ("Drqv2Aug", {}), ("HorizontalFlipAug", {})],
                            B=4, c=9, hw=32, both=False, base_seed=304),
}
CASES = {**SINGLES, **CHAINS}

# learning_utils.sample_move_and_augment of the reference on a reference ReplayBuffer of uint8 frames
SMAA = dict(name="aug_smaa", members=[("TranslateAug", {}), ("CutoutColorAug", dict(_SMALL_BOX)), ("VerticalFlipAug", {})],
            B=8, c=3, hw=24, rows=24, act=2, mixes=(0.0, 0.5, 1.0), seed=401)

# one critic_update of an existing pixel case (synth.CASES["drqv2_pixels"]: 9 x 84 x 84 uint8 frames, B 8) with a three-member
# chain as the augmenter at aug_mix 0.5.  A whole observation batch is larger than a fixture may be, so the reference's
# primary batch is recorded as its AUGMENTED rows (the first int(B * aug_mix)), s in one file and s' in another; the rows
# behind them are the replay rows themselves (regenerated from the case's seed and the recorded indices).
CRITIC = dict(name="aug_critic_update", case="drqv2_pixels", aug_mix=0.5, seed=402,
              members=[("TranslateAug", {}), ("CutoutColorAug", {}), ("HorizontalFlipAug", {})])
CRITIC_FILES = ("aug_critic_update", "aug_critic_update_s1")


def is_exact(spec):
    """integer-valued outputs (stored as uint8): everything but Gamma and the DrQv2 bilinear shift"""
    return not any(cls in ("GammaAug", "Drqv2Aug") for cls, _ in spec["members"])


def images(seed, B, c, hw):
    """seeded uint8 image batch with a share of exact zeros (what a negative gamma turns into 255)"""
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (B, c, hw, hw)).astype(np.uint8)
    img[rs.rand(B, c, hw, hw) < 0.08] = 0
    return img


def smaa_transitions(spec=SMAA):
    rs = np.random.RandomState(spec["seed"])
    n, c, hw = spec["rows"], spec["c"], spec["hw"]
    s = {"obs": rs.randint(0, 256, (n, c, hw, hw)).astype(np.uint8)}
    s1 = {"obs": rs.randint(0, 256, (n, c, hw, hw)).astype(np.uint8)}
    a = rs.uniform(-1, 1, (n, spec["act"])).astype(np.float32)
    r = rs.randn(n, 1).astype(np.float32)
    d = (rs.rand(n, 1) < 0.1)
    return s, a, r, s1, d


def build(mod, spec):
    """the case's augmentations from `mod` (the reference's augmentations module, or super_sac_amd.augmentations)"""
    return [getattr(mod, cls)(spec["B"], **kw) for cls, kw in spec["members"]]


def snapshot(augs, spec):
    out = {}
    for j, (aug, (cls, _)) in enumerate(zip(augs, spec["members"])):
        for attr in STATE[cls]:
            v = getattr(aug, attr)
            out[f"p{j}_{attr}"] = v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v).copy()
    return out


def _hook_value(cls, rec, j):
    def t(attr):
        return torch.from_numpy(np.array(rec[f"p{j}_{attr}"]))
    if cls in ("CutoutAug", "WindowAug"):
        return t("w1"), t("h1")
    if cls == "CutoutColorAug":
        return t("w1"), t("h1"), t("rand_box")
    if cls in ("TranslateAug", "LargeTranslateAug"):
        return t("translation"), t("random_color")
    if cls in ("HorizontalFlipAug", "VerticalFlipAug"):
        return np.array(rec[f"p{j}_random_inds"])
    if cls == "RotateAug":
        return t("random_inds")
    if cls == "GammaAug":
        return t("gamma")
    if cls == "Drqv2Aug":
        return t("shift")
    raise KeyError(cls)


class DrawReplay:
    """replaces the rng.draw_* hooks of the case's classes so that the NEXT randomisation of member j returns the recorded
    parameters (members that share a hook are served in sequence order, as AugmentationSequence randomises them)"""

    def __init__(self, rng_mod, spec, rec, repeat=1):
        self.rng, self.saved, self.queues = rng_mod, {}, {}
        for _ in range(repeat):
            for j, (cls, _kw) in enumerate(spec["members"]):
                self.queues.setdefault(HOOK[cls], []).append(_hook_value(cls, rec, j))

    def __enter__(self):
        for hook, queue in self.queues.items():
            self.saved[hook] = getattr(self.rng, hook)
            setattr(self.rng, hook, lambda *a, _q=queue, **k: _q.pop(0))
        return self

    def __exit__(self, *exc):
        for hook, fn in self.saved.items():
            setattr(self.rng, hook, fn)


def set_state(augs, spec, rec):
    """put the recorded randomisation into already built objects (no draw)"""
    for j, (aug, (cls, _)) in enumerate(zip(augs, spec["members"])):
        vals = _hook_value(cls, rec, j)
        vals = vals if isinstance(vals, tuple) else (vals,)
        for attr, v in zip(STATE[cls], vals):
            setattr(aug, attr, v)
        aug._adopt_state()


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- a numpy restatement of what ssac_aug_chain does with an op table (include/ssac_hip.h), for the CPU tests:
# the host-built table is checked against the reference's outputs without a GPU
def walk_table(table, img):
    """table: (B, n_ops, 8) int32 as _ChainPlan.host_table() builds it; img: (B, c, h, w) array -> float32 output"""
    B, c, h, w = img.shape
    tabf = table.view(np.float32)
    out = np.zeros((B, c, h, w), np.float32)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for b in range(B):
        for ch in range(c):
            yy, xx = ys.copy(), xs.copy()
            stop = np.full((h, w), -1)
            live = np.ones((h, w), bool)
            for j in range(table.shape[1] - 1, -1, -1):
                op, i0, i1, i2, i3 = (int(v) for v in table[b, j, :5])
                fill = np.zeros((h, w), bool)
                if op in (1, 2):
                    fill = (yy >= i0) & (yy < i1) & (xx >= i2) & (xx < i3) & (op == 1 or ch < 3 * (c // 3))
                elif op == 3:
                    yy, xx = np.where(live, yy - i0, yy), np.where(live, xx - i1, xx)
                    fill = (yy < 0) | (yy >= h) | (xx < 0) | (xx >= w)
                elif op == 4:
                    xx = np.where(live, w - 1 - xx, xx)
                elif op == 5:
                    yy = np.where(live, h - 1 - yy, yy)
                elif op == 6:
                    if i0 == 2:
                        ny, nx = h - 1 - yy, w - 1 - xx
                    elif i0 == 1:
                        ny, nx = xx, w - 1 - yy
                    elif i0 == 3:
                        ny, nx = h - 1 - xx, yy
                    else:
                        ny, nx = yy, xx
                    yy, xx = np.where(live, ny, yy), np.where(live, nx, xx)
                elif op == 7:
                    fill = (yy < i0) | (yy >= i0 + i2) | (xx < i1) | (xx >= i1 + i2)
                fill = fill & live
                stop[fill] = j
                live = live & ~fill
            val = np.zeros((h, w), np.float32)
            val[live] = img[b, ch][yy[live], xx[live]].astype(np.float32)
            for j in range(table.shape[1]):
                if table[b, j, 0] in (2, 3):
                    val[stop == j] = tabf[b, j, 5 + ch % 3]
            for j in range(table.shape[1]):
                if table[b, j, 0] == 8:
                    m = stop < j
                    x = (val[m] / np.float32(255.0)).astype(np.float32)
                    with np.errstate(divide="ignore", over="ignore"):
                        p = np.power(x.astype(np.float64), np.float64(tabf[b, j, 5])).astype(np.float32)
                    val[m] = np.clip(p * np.float32(255.0), 0.0, 255.0).astype(np.float32)
            out[b, ch] = val
    return out
