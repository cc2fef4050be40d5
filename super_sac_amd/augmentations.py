"""Augmentations on the device (mirror of super_sac/augmentations.py).  One randomisation per call is
shared by every batch passed (s and s' get the same shift / box / flip ...).

DrQ family (augmentations.py:165-293): the ``ssac_drq_shift`` kernel.  Cutout, cutout-color, translate, flips,
rotate, window and gamma (augmentations.py:83-126, 296-534): the ``ssac_aug_chain`` kernel, which evaluates a
whole sequence of them in one pass (a per-row op table, built on the host from the reference's draws and uploaded
once per randomisation).  Colour jitter and network randomisation (augmentations.py:537-801) are neither an index map nor a
fill: each is a device pass of its own (``ssac_aug_colour_jitter``, ``ssac_aug_netrand``; one workgroup per row and group of
three channels).  When used through ``learning_utils.sample_move_and_augment`` every kernel reads the uint8 replay rows
directly (gather + uint8->fp32 + augmentation + aug_mix row selection fused, one pass over the pixels).

ColorJitterAug also draws at APPLICATION time (the row selection and the contrast / HSV order, per frame group): a sequence
that holds one draws the orders of a whole call up front, in the reference's order (``AugmentationSequence.draw_orders``).

Not covered (``adopt.adopt_augmenter`` says why): GrayscaleAug, RadAug.
"""
import numbers

import numpy as np
import torch

from . import engine, rng
from ._lib import check, lib


class _ShiftAug:
    MODE = 0

    def __init__(self, batch_size, pad=4, noise=False, *_a, **_k):
        self.batch_size, self.pad, self.noise = batch_size, pad, noise
        self._shift_dev = None
        self.change_randomization_params()

    def _upload(self, shift_xy):
        self._shift_host = shift_xy.contiguous()
        self._shift_dev = None

    def _adopt_state(self):
        """an object built by the reference's class of the same name (adopt.adopt_augmenter swapped its class): take
        over the randomisation it currently holds, without drawing"""
        raise NotImplementedError

    def shift_device(self, device):
        if self._shift_dev is None or self._shift_dev.device != device:
            self._shift_dev = self._shift_host.to(device)
        return self._shift_dev

    def apply(self, src, idx, n, c, h, n_aug, dst, noise=None):
        assert n == self.batch_size
        check(lib.ssac_drq_shift(src.data_ptr(), 1 if src.dtype == torch.uint8 else 0,
                                 0 if idx is None else idx.data_ptr(), n, c, h, self.pad,
                                 self.shift_device(dst.device).data_ptr(), self.MODE,
                                 0 if noise is None else noise.data_ptr(), n_aug, dst.data_ptr(),
                                 engine.stream()))
        return dst

    def __call__(self, imgs):
        engine.require_gpu(imgs)
        n, c, h, w = imgs.shape
        assert h == w
        assert n == self.batch_size
        imgs = imgs.contiguous()
        noise = rng.draw_normal((n, c, h, w), imgs.device) if self.noise else None
        return self.apply(imgs, None, n, c, h, n, torch.empty_like(imgs, dtype=torch.float32), noise)


class Drqv2Aug(_ShiftAug):
    """replicate-pad + bilinear grid shift (augmentations.py:214-269)."""
    MODE = 0

    def change_randomization_params(self):
        self.shift = rng.draw_drqv2_shift(self.batch_size, self.pad)  # (B,1,1,2): x, y
        self._upload(self.shift.reshape(self.batch_size, 2).to(torch.int64))

    def _adopt_state(self):
        self._upload(self.shift.reshape(self.batch_size, 2).to(torch.int64))

    def __repr__(self):
        return "DrqV2"


class DrqAug(_ShiftAug):
    """reflection-pad + integer crop (+ N(0,1) noise) (augmentations.py:165-211)."""
    MODE = 1

    def __init__(self, batch_size, pad=4, noise=True, *_a, **_k):
        super().__init__(batch_size, pad, noise)

    def change_randomization_params(self):
        self.w1, self.h1 = rng.draw_drq_offsets(self.batch_size, self.pad)
        self._upload(torch.stack([self.w1, self.h1], dim=1).to(torch.int64))

    def _adopt_state(self):
        self._upload(torch.stack([self.w1, self.h1], dim=1).to(torch.int64))

    def __repr__(self):
        return "Drqv1"


class DrqNoNoiseAug(DrqAug):
    def __init__(self, batch_size, pad=4, noise=False, *_a, **_k):
        super().__init__(batch_size, pad, noise)

    def __repr__(self):
        return "Drqv1NoNoise"


class LargeDrqNoNoiseAug(DrqAug):
    def __init__(self, batch_size, pad=12, noise=False, *_a, **_k):
        super().__init__(batch_size, pad, noise)

    def __repr__(self):
        return "Drqv1LargeNoNoise"


class LargeDrqAug(DrqAug):
    def __init__(self, batch_size, pad=12, *_a, **_k):
        super().__init__(batch_size, pad)

    def __repr__(self):
        return "Drqv1Large"


class IdentityAug:
    def __init__(self, batch_size, *_a, **_k):
        self.batch_size = batch_size

    def __call__(self, imgs):
        return imgs

    def change_randomization_params(self):
        return

    def _adopt_state(self):
        return

    def __repr__(self):
        return "Identity"


# ------------------------------------------------------------------------------------------ chained augmentations
# opcodes and the 8-word op record of include/ssac_hip.h (struct ssac_aug_op: op, i0..i3 int32, f0..f2 float)
AUG_NOP, AUG_CUTOUT, AUG_CUTOUT_COLOR, AUG_TRANSLATE, AUG_HFLIP, AUG_VFLIP, AUG_ROTATE, AUG_WINDOW, AUG_GAMMA = range(9)
AUG_MAX_OPS = 8
_OP_WORDS = 8


class _ChainAug:
    """an augmentation that is one op per row of the ``ssac_aug_chain`` table: the randomisation lives in the attributes
    the reference's class of the same name keeps (REF_STATE), drawn by the rng.draw_* hooks on the reference's generators.
    A _ChainPlan keeps the uploaded table until a member's state changes: through change_randomization_params() /
    _adopt_state(), or by ASSIGNING a new object to one of the REF_STATE attributes (``aug.w1 = ...``, as the reference's
    objects allow).  Writing INTO such a tensor in place is not seen; call _bump() after it."""
    REF_STATE = ()

    def _state_key(self):
        return (self.__dict__.get("_version", 0),) + tuple(id(self.__dict__.get(n)) for n in self.REF_STATE)

    def _bump(self):
        # (a _ChainPlan caches the uploaded table until one of its members changes)
        self._version = self.__dict__.get("_version", 0) + 1

    def _adopt_state(self):
        """an object built by the reference's class of the same name: the randomisation it holds is used as it is"""
        self._bump()

    def _fill_ops(self, ti, tf):
        """write this augmentation's op of every row: ti (B, 8) int32 and tf, the float32 view of the same words"""
        raise NotImplementedError

    def _check_shape(self, c, h, w):
        return

    def __call__(self, imgs):
        engine.require_gpu(imgs)
        n, c, h, w = imgs.shape
        return _ChainPlan([self]).apply(imgs.contiguous(), None, n, c, h, w, n,
                                        torch.empty(n, c, h, w, device=imgs.device, dtype=torch.float32))


class _ChainPlan:
    """consecutive chain augmentations as ONE ssac_aug_chain launch.  The (B, n_ops, 8) table is built on the host and
    uploaded with one copy per randomisation, whatever the number of members."""

    def __init__(self, members):
        assert 1 <= len(members) <= AUG_MAX_OPS, f"ssac_aug_chain walks at most {AUG_MAX_OPS} augmentations per launch"
        self.members = list(members)
        self.batch_size = members[0].batch_size
        assert all(m.batch_size == self.batch_size for m in members)
        self._key, self._dev = None, None

    def host_table(self):
        tab = np.zeros((self.batch_size, len(self.members), _OP_WORDS), np.int32)
        tabf = tab.view(np.float32)
        for j, m in enumerate(self.members):
            m._fill_ops(tab[:, j], tabf[:, j])
        return tab

    def table(self, device):
        key = (tuple(m._state_key() for m in self.members), device)
        if key != self._key:
            # (the state objects the key names are held while it is current, so their ids cannot be reused meanwhile)
            self._held = [m.__dict__.get(n) for m in self.members for n in m.REF_STATE]
            self._dev, self._key = torch.from_numpy(self.host_table()).to(device), key
        return self._dev

    def apply(self, src, idx, n, c, h, w, n_aug, dst):
        assert n == self.batch_size, "the randomisation was drawn for `batch_size` rows"
        assert src.dtype in (torch.uint8, torch.float32) and dst.dtype == torch.float32
        for m in self.members:
            m._check_shape(c, h, w)
        check(lib.ssac_aug_chain(src.data_ptr(), 1 if src.dtype == torch.uint8 else 0,
                                 0 if idx is None else idx.data_ptr(), n, c, h, w,
                                 self.table(dst.device).data_ptr(), len(self.members), len(self.members), n_aug,
                                 dst.data_ptr(), engine.stream()))
        return dst


class _DevicePasses:
    """a sequence as device passes: one ssac_aug_chain launch per run of chain augmentations, one ssac_drq_shift launch
    per DrQ-family member, one ssac_aug_colour_jitter / ssac_aug_netrand launch per colour member.  The first pass reads the
    source (replay rows through idx), later ones a temporary -- an index map cannot run in place.  A DrQ member that adds
    noise is refused in a mixed sequence: its N(0, 1) draws come from
    the device generator, and no recorded reference output pins how they interleave with the other members' passes."""

    def __init__(self, aug_list):
        noisy = [a for a in aug_list if isinstance(a, _ShiftAug) and a.noise]
        if noisy:
            raise NotImplementedError(f"{noisy[0]!r} with noise inside a sequence of chained augmentations has no HIP path; "
                                      "use its noise-free variant (DrqNoNoiseAug, LargeDrqNoNoiseAug, Drqv2Aug)")
        self.passes, run = [], []
        for a in aug_list:
            if isinstance(a, _ChainAug):
                run.append(a)
                continue
            if run:
                self.passes.append(_ChainPlan(run))
                run = []
            self.passes.append(a)
        if run:
            self.passes.append(_ChainPlan(run))

    def run(self, src, idx, n, c, h, w, n_aug, device, orders=None):
        """orders: the contrast-first bit masks of this application, one per ColorJitterAug pass in pass order
        (AugmentationSequence.draw_orders); None: each such pass draws its own now, as a stand-alone call does"""
        cur, cur_idx = src, idx
        jitters = 0
        for p in self.passes:
            out = torch.empty(n, c, h, w, device=device, dtype=torch.float32)
            if isinstance(p, _ShiftAug):
                assert h == w
                p.apply(cur, cur_idx, n, c, h, n_aug, out, None)
            elif isinstance(p, ColorJitterAug):
                p.apply(cur, cur_idx, n, c, h, w, n_aug, out, None if orders is None else orders[jitters])
                jitters += 1
            else:
                p.apply(cur, cur_idx, n, c, h, w, n_aug, out)
            cur, cur_idx = out, None
        return cur


def _box_ops(ti, op, pivot_h, pivot_w, w1, h1):
    h1, w1 = np.asarray(h1, np.int64), np.asarray(w1, np.int64)
    r0, c0 = pivot_h + h1, pivot_w + w1
    if (r0 < 0).any() or (c0 < 0).any():
        raise ValueError("cutout box starting at a negative row / column")
    ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3], ti[:, 4] = op, r0, r0 + h1, c0, c0 + w1


class CutoutAug(_ChainAug):
    """rows [pivot_h + h1, pivot_h + 2 h1) x columns [pivot_w + w1, pivot_w + 2 w1) of every channel become 0, clipped at
    the image edge like the reference's slice (augmentations.py:83-126)."""
    REF_STATE = ("box_min", "box_max", "pivot_h", "pivot_w", "w1", "h1")

    def __init__(self, batch_size, box_min=7, box_max=22, pivot_h=12, pivot_w=24, *_a, **_k):
        self.box_min, self.box_max, self.pivot_h, self.pivot_w = box_min, box_max, pivot_h, pivot_w
        self.batch_size = batch_size
        self.change_randomization_params()

    def change_randomization_params(self):
        self.w1, self.h1 = rng.draw_cutout_box(self.batch_size, self.box_min, self.box_max)
        self._bump()

    def _fill_ops(self, ti, tf):
        _box_ops(ti, AUG_CUTOUT, self.pivot_h, self.pivot_w, self.w1, self.h1)

    def __repr__(self):
        return "Cutout"


class CutoutColorAug(_ChainAug):
    """the cutout box painted ``rand_box[i, ch % 3]``, on the first 3 * (c // 3) channels only (augmentations.py:355-400)."""
    REF_STATE = ("box_min", "box_max", "pivot_h", "pivot_w", "w1", "h1", "rand_box")

    def __init__(self, batch_size, box_min=7, box_max=22, pivot_h=12, pivot_w=24, *_a, **_k):
        self.box_min, self.box_max, self.pivot_h, self.pivot_w = box_min, box_max, pivot_h, pivot_w
        self.batch_size = batch_size
        self.change_randomization_params()

    def change_randomization_params(self):
        self.w1, self.h1, self.rand_box = rng.draw_cutout_color(self.batch_size, self.box_min, self.box_max)
        self._bump()

    def _fill_ops(self, ti, tf):
        _box_ops(ti, AUG_CUTOUT_COLOR, self.pivot_h, self.pivot_w, self.w1, self.h1)
        tf[:, 5:8] = self.rand_box.detach().cpu().reshape(self.batch_size, 3).numpy()

    def __repr__(self):
        return "CutoutColor"


class TranslateAug(_ChainAug):
    """out[i, ch, y, x] = img[i, ch, y - t[i, 0], x - t[i, 1]] where that lies inside the image, else
    ``random_color[i, ch % 3]`` (augmentations.py:296-344).  The channel count must be a multiple of 3, as the
    reference's ``random_color.repeat(1, c // 3, 1, 1)`` demands."""
    REF_STATE = ("translate_max", "translation", "random_color")

    def __init__(self, batch_size, translate_max=4, *_a, **_k):
        self.batch_size = batch_size
        self.translate_max = translate_max
        self.change_randomization_params()

    def change_randomization_params(self):
        self.translation, self.random_color = rng.draw_translation(self.batch_size, self.translate_max)
        self._bump()

    def _check_shape(self, c, h, w):
        if c % 3 != 0:
            raise RuntimeError(f"{self!r}: {c} channels are not a multiple of 3 (the border colour is per RGB group)")

    def _fill_ops(self, ti, tf):
        ti[:, 0] = AUG_TRANSLATE
        ti[:, 1:3] = self.translation.detach().cpu().reshape(self.batch_size, 2).numpy()
        tf[:, 5:8] = self.random_color.detach().cpu().reshape(self.batch_size, 3).numpy()

    def __repr__(self):
        return "Translate"


class LargeTranslateAug(TranslateAug):
    def __init__(self, batch_size, translate_max=8, *_a, **_k):
        super().__init__(batch_size, translate_max)

    def __repr__(self):
        return "LargeTranslate"


class _FlipAug(_ChainAug):
    REF_STATE = ("p_flip", "dim", "random_inds")

    def __init__(self, batch_size, p_rand=0.5, dim=None, *_a, **_k):
        assert dim
        self.p_flip = p_rand
        self.batch_size = batch_size
        self.dim = dim
        self.change_randomization_params()

    def change_randomization_params(self):
        self.random_inds = rng.draw_flip_rows(self.batch_size, self.p_flip)
        self._bump()

    def _fill_ops(self, ti, tf):
        assert self.dim in (2, 3)
        ti[:, 0] = np.where(np.asarray(self.random_inds, bool), AUG_HFLIP if self.dim == 3 else AUG_VFLIP, AUG_NOP)


class HorizontalFlipAug(_FlipAug):
    """the selected rows reversed along dim 3 (augmentations.py:427-454)."""

    def __init__(self, batch_size, p_rand=0.5, *_a, **_k):
        super().__init__(batch_size, p_rand, dim=3)

    def __repr__(self):
        return "HorizontalFlip"


class VerticalFlipAug(_FlipAug):
    """the selected rows reversed along dim 2 (augmentations.py:457-462)."""

    def __init__(self, batch_size, p_rand=0.5, *_a, **_k):
        super().__init__(batch_size, p_rand, dim=2)

    def __repr__(self):
        return "VerticalFlip"


class RotateAug(_ChainAug):
    """What the reference computes, not what its name suggests (augmentations.py:465-486).  It draws
    ``random_inds = randint(4) * B + arange(B)`` and then turns the rows where ``random_inds == k`` for k = 1, 2, 3 by
    ``k + 1`` quarter turns.  So row i is turned only when ``draw_i * B + i`` itself is 1, 2 or 3: by 180 degrees for the
    value 1, by 270 degrees for 2, and not at all for 3 (four quarter turns).  With B >= 4 only rows 1 and 2 can ever turn,
    and only when their draw is 0.  The per-row turn count is computed on the host by exactly this rule (``turns()``)."""
    REF_STATE = ("random_inds",)

    def __init__(self, batch_size, *_a, **_k):
        self.batch_size = batch_size
        self.change_randomization_params()

    def change_randomization_params(self):
        self.random_inds = rng.draw_rotation(self.batch_size)
        self._bump()

    def turns(self):
        """quarter turns per row, as ``torch.rot90(k=..., dims=(2, 3))`` counts them: 0, 2 or 3"""
        v = np.asarray(self.random_inds, np.int64)
        t = np.zeros(self.batch_size, np.int32)
        for k in (1, 2, 3):
            t[v == k] = (k + 1) % 4
        return t

    def _check_shape(self, c, h, w):
        if h != w and (self.turns() % 2 == 1).any():
            raise RuntimeError("Rotate: a quarter turn of a non-square image does not fit the batch")

    def _fill_ops(self, ti, tf):
        t = self.turns()
        ti[:, 0], ti[:, 1] = np.where(t != 0, AUG_ROTATE, AUG_NOP), t

    def __repr__(self):
        return "Rotate"


class WindowAug(_ChainAug):
    """everything outside rows [h1, h1 + 64) x columns [w1, w1 + 64) becomes 0 (augmentations.py:506-534; the reference
    multiplies by a 0/1 mask, which is the same for the finite, non-negative pixel values)."""
    REF_STATE = ("crop_size", "crop_max", "w1", "h1")

    def __init__(self, batch_size, *_a, **_k):
        self.batch_size = batch_size
        self.crop_size = 64
        self.crop_max = 75 - self.crop_size
        self.change_randomization_params()

    def change_randomization_params(self):
        self.w1, self.h1 = rng.draw_window(self.batch_size, self.crop_max)
        self._bump()

    def _fill_ops(self, ti, tf):
        ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3] = AUG_WINDOW, np.asarray(self.h1), np.asarray(self.w1), self.crop_size

    def __repr__(self):
        return "Window"


class GammaAug(_ChainAug):
    """clamp(((x / 255) ** gamma_i) * 255, 0, 255) with gamma_i ~ N(1, 0.45) (augmentations.py:403-424).  A draw can be
    negative; a 0 pixel then becomes inf and the clamp makes it 255 -- kept, as the reference computes it.  The kernel
    divides in correctly rounded fp32, takes the power in fp64 rounded once to fp32, then multiplies and clamps in fp32."""
    gamma_mean = 1.0
    gamma_std = 0.45
    REF_STATE = ("gamma",)

    def __init__(self, batch_size, *_a, **_k):
        self.batch_size = batch_size
        self.change_randomization_params()

    def change_randomization_params(self):
        self.gamma = rng.draw_gamma(self.batch_size, self.gamma_mean, self.gamma_std)
        self._bump()

    def _fill_ops(self, ti, tf):
        ti[:, 0] = AUG_GAMMA
        tf[:, 5] = self.gamma.detach().cpu().reshape(self.batch_size).float().numpy()

    def __repr__(self):
        return "Gamma"


# ------------------------------------------------------------------------------------------ colour augmentations
class _ColourAug:
    """an augmentation with a kernel of its own that works on groups of three channels (csrc/ssac_aug_colour.hip): a device
    pass of its own kind in _DevicePasses.  The randomisation lives in the attributes the reference's class of the same name
    keeps (REF_STATE); its device copy is uploaded once per randomisation and kept until the state changes -- through
    change_randomization_params() / _adopt_state(), or by ASSIGNING a new object to a REF_STATE attribute.  Writing INTO such
    a tensor in place is not seen; call _bump() after it."""
    REF_STATE = ()
    NEEDS_BATCH_SIZE = True   # (adopt.adopt_augmenter: the reference's object carries `batch_size`)

    _state_key = _ChainAug._state_key
    _bump = _ChainAug._bump

    def _adopt_state(self):
        self._bump()

    def _host_params(self):
        """the float32 tensor the kernel reads"""
        raise NotImplementedError

    def _device_params(self, device):
        key = (self._state_key(), device)
        if key != self.__dict__.get("_dev_key"):
            # (the state objects the key names are held while it is current, so their ids cannot be reused meanwhile)
            self._held = [self.__dict__.get(n) for n in self.REF_STATE]
            self._dev, self._dev_key = self._host_params().contiguous().to(device), key
        return self._dev


def _jitter_range(setting, name, around, floor=None, inside=(None, None)):
    """the [lo, hi] interval a ColorJitterAug factor is drawn from, or None where the interval is the single point `around`
    (the factor would change nothing).  A scalar s stands for [around - s, around + s], its lower end cut off at `floor`
    where one is given; a pair is used as it is and has to lie within `inside`."""
    if isinstance(setting, numbers.Real):
        if setting < 0:
            raise ValueError(f"ColorJitterAug: {name}={setting!r} is a half-width and cannot be negative")
        lo, hi = around - setting, around + setting
        interval = [lo if floor is None else max(lo, floor), hi]
    else:
        try:
            lo, hi = setting
        except (TypeError, ValueError):
            raise TypeError(f"ColorJitterAug: {name} takes a half-width or a (lo, hi) pair, not {setting!r}") from None
        least, most = inside
        if not (lo <= hi and (least is None or least <= lo) and (most is None or hi <= most)):
            raise ValueError(f"ColorJitterAug: {name}={setting!r} is not an interval within {inside}")
        interval = setting
    return None if interval[0] == interval[1] == around else interval


def jitter_refusal(aug):
    """why the reference's own ColorJitterAug fails with this object's settings (None: it runs)"""
    if aug.stack_size != 1:
        return (f"stack_size = {aug.stack_size}: the reference's own class raises for every stack_size but 1 "
                "(factor.view(len(x), 1, 1, 1) of a batch_size * stack_size vector, augmentations.py:594)")
    if aug.prob != 1.0:
        return (f"p_rand = {aug.prob}: the reference's own class raises whenever a row is left out (the same view, taken on "
                "the selected rows only, augmentations.py:594-686), so only p_rand = 1.0 has an output to match")
    for name in ("contrast", "hue", "brightness", "saturation"):
        if getattr(aug, name) is None:
            return (f"{name} is a zero range (None): the reference's own class raises in uniform_(*None) "
                    "(augmentations.py:648-675)")
    return None


class ColorJitterAug(_ColourAug):
    """per-row contrast, hue, brightness and saturation factors on every group of three channels (augmentations.py:537-771):
    x / 255, then contrast = clamp((x - mean) * fc + mean) with the mean over (H, W) per image and channel and the HSV block
    (rgb2hsv, brightness, hue, saturation, hsv2rgb) in an order that is drawn PER APPLICATION AND FRAME GROUP
    (rng.draw_jitter_order), then * 255.  Channels beyond 3 * (c // 3) only make the / 255 * 255 round trip.  The quirks of
    the reference's formulas that the kernel keeps are listed in include/ssac_hip.h (ssac_aug_colour_jitter).

    Only what the reference itself can run is accepted: stack_size == 1, p_rand == 1.0 and four non-zero ranges
    (jitter_refusal)."""
    REF_STATE = ("brightness", "contrast", "saturation", "hue", "prob", "stack_size",
                 "factor_contrast", "factor_hue", "factor_brightness", "factor_saturate")
    MAX_GROUPS = 32   # SSAC_AUG_COLOUR_MAX_GROUPS: one bit per frame group

    def __init__(self, batch_size, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.5, p_rand=1.0, stack_size=1,
                 *_a, **_k):
        self.brightness = _jitter_range(brightness, "brightness", 1, floor=0, inside=(0, None))
        self.contrast = _jitter_range(contrast, "contrast", 1, floor=0, inside=(0, None))
        self.saturation = _jitter_range(saturation, "saturation", 1, floor=0, inside=(0, None))
        self.hue = _jitter_range(hue, "hue", 0, inside=(-0.5, 0.5))
        self.prob = p_rand
        self.batch_size = batch_size
        self.stack_size = stack_size
        why = jitter_refusal(self)
        if why:
            raise NotImplementedError(f"augmentation 'ColorJitterAug' has no HIP path for {why}")
        self.change_randomization_params()

    def change_randomization_params(self):
        (self.factor_contrast, self.factor_hue, self.factor_brightness,
         self.factor_saturate) = rng.draw_color_jitter(self.batch_size, self.contrast, self.hue, self.brightness,
                                                       self.saturation)
        self._bump()

    def _adopt_state(self):
        why = jitter_refusal(self)
        if why:
            raise NotImplementedError(f"augmentation 'ColorJitterAug' has no HIP path for {why}")
        self._bump()

    def _host_params(self):
        cols = [torch.as_tensor(getattr(self, n)).detach().cpu().float().reshape(self.batch_size)
                for n in ("factor_contrast", "factor_hue", "factor_brightness", "factor_saturate")]
        return torch.stack(cols, dim=1)   # (B, 4): contrast, hue, brightness, saturation

    def draw_order(self, c):
        """the draws of ONE application to a c-channel batch: bit g set = group g applies contrast before the HSV block"""
        groups = c // 3
        if groups > self.MAX_GROUPS:
            raise RuntimeError(f"{self!r}: {groups} groups of three channels, ssac_aug_colour_jitter takes {self.MAX_GROUPS}")
        bits = 0
        for g in range(groups):
            if rng.draw_jitter_order(self.batch_size, self.prob):
                bits |= 1 << g
        return bits

    def apply(self, src, idx, n, c, h, w, n_aug, dst, order=None):
        assert n == self.batch_size, "the randomisation was drawn for `batch_size` rows"
        assert src.dtype in (torch.uint8, torch.float32) and dst.dtype == torch.float32
        if order is None:
            order = self.draw_order(c)
        check(lib.ssac_aug_colour_jitter(src.data_ptr(), 1 if src.dtype == torch.uint8 else 0,
                                         0 if idx is None else idx.data_ptr(), n, c, h, w,
                                         self._device_params(dst.device).data_ptr(), order, n_aug, dst.data_ptr(),
                                         engine.stream()))
        return dst

    def __call__(self, imgs):
        engine.require_gpu(imgs)
        n, c, h, w = imgs.shape
        return self.apply(imgs.contiguous(), None, n, c, h, w, n,
                          torch.empty(n, c, h, w, device=imgs.device, dtype=torch.float32))

    def __repr__(self):
        return "ColorJitter"


def _conv_holding(weight):
    """a Conv2d(3, 3, 3, bias=False, padding=1) around `weight` (what the reference keeps as ``conv``), built without
    touching any generator"""
    conv = torch.nn.utils.skip_init(torch.nn.Conv2d, 3, 3, kernel_size=3, bias=False, padding=1)
    conv.weight.data = torch.as_tensor(weight).detach().float().reshape(3, 3, 3, 3)
    return conv


class NetworkRandomizationAug(_ColourAug):
    """one random Conv2d(3, 3, 3, bias=False, padding=1) per randomisation, the same for every row, on every group of three
    channels of x / 255; times 255, NOT clamped -- outputs leave [0, 255], as the reference's do (augmentations.py:774-801).
    Like the reference's object it keeps ``conv`` and nothing else: no batch size."""
    REF_STATE = ("conv",)
    NEEDS_BATCH_SIZE = False

    def __init__(self, batch_size=None, *_a, **_k):
        self.change_randomization_params()

    def change_randomization_params(self):
        self.conv = _conv_holding(rng.draw_netrand_conv())
        self._bump()

    def _adopt_state(self):
        # (an object built by the reference's class is a torch.nn.Module: it keeps `conv` among its sub-modules)
        mods = self.__dict__.get("_modules")
        if "conv" not in self.__dict__ and mods and "conv" in mods:
            self.__dict__["conv"] = mods["conv"]
        self._bump()

    def _host_params(self):
        return self.conv.weight.detach().cpu().float().reshape(81)   # [co][ci][ky][kx]

    def apply(self, src, idx, n, c, h, w, n_aug, dst):
        assert src.dtype in (torch.uint8, torch.float32) and dst.dtype == torch.float32
        check(lib.ssac_aug_netrand(src.data_ptr(), 1 if src.dtype == torch.uint8 else 0,
                                   0 if idx is None else idx.data_ptr(), n, c, h, w,
                                   self._device_params(dst.device).data_ptr(), n_aug, dst.data_ptr(), engine.stream()))
        return dst

    def __call__(self, imgs):
        engine.require_gpu(imgs)
        n, c, h, w = imgs.shape
        return self.apply(imgs.contiguous(), None, n, c, h, w, n,
                          torch.empty(n, c, h, w, device=imgs.device, dtype=torch.float32))


class AugmentationSequence:
    def __init__(self, aug_list, keys=None):
        self.aug_list = aug_list
        self.keys = keys

    def is_identity(self):
        return all(isinstance(a, IdentityAug) for a in self.aug_list)

    def single_shift(self):
        """the one shift-type augmentation this sequence consists of (fusable), else None."""
        real = [a for a in self.aug_list if not isinstance(a, IdentityAug)]
        return real[0] if len(real) == 1 and isinstance(real[0], _ShiftAug) else None

    def _real(self):
        return [a for a in self.aug_list if not isinstance(a, IdentityAug)]

    def device_chain(self):
        """the fused plan (one ssac_aug_chain launch per batch) when every non-identity member is a chain augmentation,
        else None"""
        passes = self.device_passes()
        if passes is not None and len(passes.passes) == 1 and isinstance(passes.passes[0], _ChainPlan):
            return passes.passes[0]
        return None

    def device_passes(self):
        """the sequence as device passes (_DevicePasses) when it holds a chain or colour augmentation and every non-identity
        member has a kernel, else None.  Cached while the members stay the same objects."""
        real = self._real()
        if (not any(isinstance(a, (_ChainAug, _ColourAug)) for a in real)
                or not all(isinstance(a, (_ChainAug, _ShiftAug, _ColourAug)) for a in real)):
            return None
        cached = self.__dict__.get("_passes")
        if cached is None or len(cached[0]) != len(real) or any(a is not b for a, b in zip(cached[0], real)):
            cached = self.__dict__["_passes"] = (real, _DevicePasses(real))
        return cached[1]

    def change_randomization_params(self):
        for aug in self.aug_list:
            aug.change_randomization_params()

    def draw_orders(self, *channels):
        """the APPLICATION-time draws of one call, made up front: ColorJitterAug draws its row selection and its contrast /
        HSV order per application and per frame group (rng.draw_jitter_order), and the reference consumes those draws
        batch-major (s, then s'), then key in ``self.keys`` order, then member, then frame group (augmentations.py:31-36).
        `channels`: one {key: channel count} dict per batch, its 4-D (image) keys.  Returns None when no member draws at
        application time, else one {key: (bit mask per ColorJitterAug member)} dict per batch; a key outside ``self.keys``
        is not augmented and draws nothing (masks of 0).  Needs no GPU."""
        jitters = [a for a in self.aug_list if isinstance(a, ColorJitterAug)]
        if not jitters:
            return None
        out = []
        for chan in channels:
            keys = list(chan) if self.keys is None else [k for k in self.keys if k in chan]
            per_key = {k: (0,) * len(jitters) for k in chan}
            for k in keys:
                per_key[k] = tuple(j.draw_order(chan[k]) for j in jitters)
            out.append(per_key)
        return out

    def _augment_one(self, batch, orders=None):
        """one observation dict through every augmentation, key by key; keys outside `self.keys` pass through as copies"""
        out = {}
        passes = self.device_passes()
        for name, value in batch.items():
            if name in self.keys and passes is not None and value.dim() == 4:
                engine.require_gpu(value)
                n, c, h, w = value.shape
                value = passes.run(value.contiguous(), None, n, c, h, w, n, value.device,
                                   None if orders is None else orders[name])
            else:
                value = value.clone()
                if name in self.keys:
                    for aug in self.aug_list:
                        value = aug(value)
            out[name] = value
        return out

    def __call__(self, *batches):
        """augmentations.py:20-38 as a contract: ONE randomisation per call, shared by every batch passed (s and s' get the
        same shift); the batches themselves are left untouched; one batch in -> one dict out, several -> a tuple."""
        if self.keys is None:   # (first call: every key of the first batch, remembered -- as the reference does)
            self.keys = batches[0].keys()
        self.change_randomization_params()
        orders = None
        if self.device_passes() is not None:
            orders = self.draw_orders(*({k: v.shape[1] for k, v in b.items() if v.dim() == 4} for b in batches))
        augmented = tuple(self._augment_one(b, None if orders is None else orders[i]) for i, b in enumerate(batches))
        return augmented[0] if len(augmented) == 1 else augmented

    def __repr__(self):
        names = [repr(a) for a in self.aug_list]
        return f"AugmentationSequence: ({names})"
