"""Write the colour-augmentation fixtures under tests/golden by driving the UNMODIFIED reference; dev container only.

    python tools/gen_aug_colour_golden.py            # every case of tests/aug_colour_cases.py
    python tools/gen_aug_colour_golden.py --out DIR  # somewhere else (tests/test_aug_colour_fixtures_cpu.py)

Three groups (tests/aug_colour_cases.py):
  1. ColorJitterAug and NetworkRandomizationAug alone: 3 channels with s and s' through ONE AugmentationSequence call, 9
     channels, and an odd 7 x 17 x 19 batch;
  2. each of them between two chain augmentations (three device passes);
  3. the reference's learning_utils.sample_move_and_augment on a reference ReplayBuffer of uint8 frames with
     [ColorJitterAug, TranslateAug], aug_mix 0 / 0.5 / 1.

Each file holds the inputs, every drawn parameter (``p{j}_{attribute}`` of member j, read off the reference's objects after
the call; ``p{j}_conv`` is the convolution's weight), the reference's fp32 outputs and ``ref_dev64``: the largest distance of
a reference output from the fp64 restatement of tests/aug_colour_cases.py, on the 0..255 scale.  ColorJitterAug draws the
order of its two stages per APPLICATION and frame group, inside forward(): a spy on ``random.uniform`` -- it calls the
original, so the generator is consumed as without it -- records them as ``order{k}`` (members x groups) of batch k.
``probe_*`` are draws taken from the torch, numpy and Python generators right after the call.
The jitter images carry planted blocks (grey, black, r == g > b, g == b > r, white, a saturated primary): asserted below.
The seed of a case is searched from its base seed until the case shows what it is there for.  Running the script twice
writes identical files.
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
import aug_colour_cases as cc  # noqa: E402
from gen_aug_golden import MAX_BYTES, probes, seed_all  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
JITTER_DEV_MAX = 1e-3   # measured 1.1e-4 .. 1.9e-4 for the reference against fp64; no element may need an exclusion


class OrderSpy:
    """records what ``random.uniform`` returns while the reference runs (ColorJitterAug.transform is its only caller)"""

    def __enter__(self):
        self.values, self.real = [], random.uniform

        def spy(a, b):
            v = self.real(a, b)
            self.values.append(v)
            return v
        random.uniform = spy
        return self

    def __exit__(self, *exc):
        random.uniform = self.real

    def flags(self, n_batches, n_members, groups):
        """(batches, members, groups): one key, so the reference's order is batch-major, member, group"""
        assert len(self.values) == n_batches * n_members * groups, (len(self.values), n_batches, n_members, groups)
        return (np.array(self.values) >= 0.5).reshape(n_batches, n_members, groups)


def _n_jitter(spec):
    return sum(cls == "ColorJitterAug" for cls, _ in spec["members"])


def shows_its_point(name, spec, params, orders):
    for j, (cls, _kw) in enumerate(spec["members"]):
        if cls in ("HorizontalFlipAug", "VerticalFlipAug"):
            sel = params[f"p{j}_random_inds"]
            if sel.all() or not sel.any():
                return False
        if cls == "TranslateAug" and not np.asarray(params[f"p{j}_translation"]).any():
            return False
    if name == "aug_jitter_c3":
        return bool(orders[0, 0, 0] != orders[1, 0, 0])          # s and s' share the factors, not the order
    if _n_jitter(spec) and cc.n_groups(spec) > 1:
        return bool(orders[0].any() and not orders[0].all())     # both orders among the groups
    return True


def run_case(ref, name, spec):
    A = ref.augmentations
    B, c, h, w = spec["B"], spec["c"], spec["h"], spec["w"]
    n_b, n_j = (2 if spec["both"] else 1), _n_jitter(spec)
    for seed in range(spec["base_seed"] * 1000, spec["base_seed"] * 1000 + 1000):
        seed_all(seed)
        augs = cc.build(A, spec)
        seq = A.AugmentationSequence(augs)
        imgs = [cc.images(seed + 1 + k, B, c, h, w) for k in range(n_b)]
        batches = [{"obs": torch.from_numpy(im).float()} for im in imgs]
        with OrderSpy() as spy:
            outs = seq(*batches)
        outs = outs if isinstance(outs, tuple) else (outs,)
        params = cc.snapshot(augs, spec)
        pr = probes()
        orders = spy.flags(n_b, n_j, cc.n_groups(spec)) if n_j else None
        if shows_its_point(name, spec, params, orders):
            break
    else:
        raise AssertionError(f"{name}: no seed shows what the case is there for")
    for b, im in zip(batches, imgs):   # the sequence left its inputs alone
        assert np.array_equal(b["obs"].numpy(), im.astype(np.float32))
    rec = {"seed": np.int64(seed), **params, **pr}
    dev = 0.0
    for k, (im, o) in enumerate(zip(imgs, outs)):
        o = o["obs"].numpy()
        assert o.dtype == np.float32 and o.shape == im.shape and np.isfinite(o).all()
        if n_j:
            assert cc.planted_present(im), name
            rec[f"order{k}"] = orders[k]
        rec[f"in{k}"], rec[f"out{k}"] = im, o
        dev = max(dev, float(np.abs(o.astype(np.float64) - cc.restate(spec, rec, k)).max()))
    rec["ref_dev64"] = np.float64(dev)
    return rec


def run_smaa(ref, spec):
    A, rlu = ref.augmentations, ref.learning_utils
    seed_all(spec["seed"])
    buf = ref.replay.ReplayBuffer(spec["rows"])
    s, a, r, s1, d = cc.smaa_transitions(spec)
    assert cc.planted_present(s["obs"]) and cc.planted_present(s1["obs"])
    buf.load_experience(s, a, r, s1, d)
    augs = cc.build(A, spec)
    seq = A.AugmentationSequence(augs)
    rec, dev = {}, 0.0
    for m, mix in enumerate(spec["mixes"]):
        with OrderSpy() as spy:
            dct = rlu.sample_move_and_augment(buf, spec["B"], seq, mix, per=False)
        idx = np.asarray(dct["priority_idxs"]).astype(np.int64)
        sub = dict(cc.snapshot(augs, spec), idx=idx)
        orders = spy.flags(2, _n_jitter(spec), cc.n_groups(spec))
        sub["order0"], sub["order1"] = orders[0], orders[1]
        o, a_, r_, o1, dn = dct["primary_batch"]
        k_aug = int(spec["B"] * mix)
        for tag, got, rows, k in (("o", o["obs"], s["obs"], 0), ("o1", o1["obs"], s1["obs"], 1)):
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and np.isfinite(got).all()
            assert np.array_equal(got[k_aug:], rows[idx[k_aug:]].astype(np.float32))   # the rows behind the mix: replay rows
            want = cc.restate(spec, sub, k, img=rows[idx])
            dev = max(dev, float(np.abs(got[:k_aug].astype(np.float64) - want[:k_aug]).max()) if k_aug else 0.0)
            sub[tag] = got
        sub["a"], sub["r"], sub["d"] = a_.cpu().numpy(), r_.cpu().numpy(), dn.cpu().numpy()
        rec.update({f"m{m}_{k}": v for k, v in sub.items()})
    rec.update(probes())
    rec["ref_dev64"] = np.float64(dev)
    return rec


def main(names=None, out=OUT):
    ref = ref_harness.import_reference()
    torch.set_num_threads(1)
    os.makedirs(out, exist_ok=True)
    todo = {**cc.CASES, cc.SMAA["name"]: cc.SMAA}
    for name in names or sorted(todo):
        spec = todo[name]
        rec = run_smaa(ref, spec) if name == cc.SMAA["name"] else run_case(ref, name, spec)
        dev = float(rec["ref_dev64"])
        print(f"   {name}: ref_dev64 {dev:.3e}")
        if _n_jitter(spec):
            assert dev < JITTER_DEV_MAX, f"{name}: the reference is {dev:.3e} away from the fp64 restatement"
        path = os.path.join(out, f"{name}.npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        print(f"   {path}: {size} bytes")
        assert size <= MAX_BYTES, f"{name}: {size} bytes"


if __name__ == "__main__":
    args = sys.argv[1:]
    out = OUT
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    main(args or None, out)
