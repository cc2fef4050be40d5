"""Write tests/golden/aug_*.npz by driving the UNMODIFIED reference's augmentations; dev container only.

    python tools/gen_aug_golden.py            # every case of tests/aug_cases.py
    python tools/gen_aug_golden.py --out DIR  # somewhere else (the determinism test)

Three groups (tests/aug_cases.py):
  1. every chain class alone (CutoutAug ... GammaAug) on a 9-channel and a 3-channel square uint8-valued batch, s and s'
     through ONE AugmentationSequence call, so the shared randomisation is on record;
  2. chains of three and more members, one of them mixed with Drqv2Aug;
  3. the reference's learning_utils.sample_move_and_augment on a reference ReplayBuffer of uint8 frames, aug_mix 0 / 0.5 / 1,
     and (aug_cases.CRITIC, the augmented rows) on the buffer of an existing pixel case with a three-member chain.

Each file holds the inputs, every drawn parameter (``p{j}_{attribute}`` of member j, read off the reference's objects after
the call) and the reference's outputs (uint8 where they are integer-valued).  ``probe_*`` are draws taken from the torch,
numpy and Python generators right after the call: a port that consumes the generators in the same order reproduces them.
The seed of a case is searched from its base seed until the case shows what it is there for (asserted below): every Rotate
turn count, flipped and unflipped rows, a cutout box clipped by the edge, a negative gamma on 0-valued pixels.
Running the script twice writes identical files.
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_harness  # noqa: E402
import aug_cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 359 * 1024   # no file larger than the largest fixture that was here before (beta_sunrise.npz)


def seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def probes():
    return {"probe_torch": torch.randint(1 << 30, (4,)).numpy(), "probe_numpy": np.random.randint(1 << 30, size=4),
            "probe_python": np.float64(random.random())}


def rotate_turns(random_inds):
    """what RotateAug.__call__ does with its values (augmentations.py:470-474), restated for the assertion only"""
    v = np.asarray(random_inds)
    t = np.zeros(len(v), np.int64)
    for k in (1, 2, 3):
        t[v == k] = (k + 1) % 4
    return t


def shows_its_point(spec, params, imgs):
    """the conditions a case's seed is searched for"""
    hw = spec["hw"]
    for j, (cls, kw) in enumerate(spec["members"]):
        if cls == "RotateAug" and set(rotate_turns(params[f"p{j}_random_inds"])) != {0, 2, 3}:
            return False
        if cls in ("HorizontalFlipAug", "VerticalFlipAug"):
            sel = params[f"p{j}_random_inds"]
            if sel.all() or not sel.any():
                return False
        if cls in ("CutoutAug", "CutoutColorAug") and len(spec["members"]) == 1:
            ph, pw = kw.get("pivot_h", 12), kw.get("pivot_w", 24)
            h1, w1 = params[f"p{j}_h1"], params[f"p{j}_w1"]
            clipped = ((ph + h1 < hw) & (ph + 2 * h1 > hw)) | ((pw + w1 < hw) & (pw + 2 * w1 > hw))
            inside = (ph + 2 * h1 <= hw) & (pw + 2 * w1 <= hw)
            # (the default pivots cannot reach the edge of the large image: that case shows whole boxes, the small one clipped ones)
            if not (inside.any() if hw > 64 else clipped.any()):
                return False
        if cls == "GammaAug":
            g = params[f"p{j}_gamma"].reshape(-1)
            if not (g < 0).any() or not all((im[g < 0] == 0).any() for im in imgs):
                return False
    return True


def run_case(ref, name, spec):
    A = ref.augmentations
    B, c, hw = spec["B"], spec["c"], spec["hw"]
    for seed in range(spec["base_seed"] * 1000, spec["base_seed"] * 1000 + 1000):
        seed_all(seed)
        augs = aug_cases.build(A, spec)
        seq = A.AugmentationSequence(augs)
        imgs = [aug_cases.images(seed + 1 + k, B, c, hw) for k in range(2 if spec["both"] else 1)]
        batches = [{"obs": torch.from_numpy(im).float()} for im in imgs]
        outs = seq(*batches)
        outs = outs if isinstance(outs, tuple) else (outs,)
        params = aug_cases.snapshot(augs, spec)
        pr = probes()
        if shows_its_point(spec, params, imgs):
            break
    else:
        raise AssertionError(f"{name}: no seed shows what the case is there for")
    assert shows_its_point(spec, params, imgs)
    for b, im in zip(batches, imgs):   # the sequence left its inputs alone
        assert np.array_equal(b["obs"].numpy(), im.astype(np.float32))
    rec = {"seed": np.int64(seed), **params, **pr}
    for k, (im, o) in enumerate(zip(imgs, outs)):
        o = o["obs"].numpy()
        assert o.dtype == np.float32 and o.shape == im.shape and np.isfinite(o).all()
        if aug_cases.is_exact(spec):
            assert np.array_equal(o, np.round(o)) and o.min() >= 0 and o.max() <= 255
            o = o.astype(np.uint8)
        rec[f"in{k}"], rec[f"out{k}"] = im, o
    return rec


def run_smaa(ref, spec):
    A, rlu = ref.augmentations, ref.learning_utils
    seed_all(spec["seed"])
    buf = ref.replay.ReplayBuffer(spec["rows"])
    buf.load_experience(*aug_cases.smaa_transitions(spec))
    augs = aug_cases.build(A, spec)
    seq = A.AugmentationSequence(augs)
    rec = {}
    for m, mix in enumerate(spec["mixes"]):
        d = rlu.sample_move_and_augment(buf, spec["B"], seq, mix, per=False)
        rec[f"m{m}_idx"] = np.asarray(d["priority_idxs"]).astype(np.int64)
        for k, v in aug_cases.snapshot(augs, spec).items():
            rec[f"m{m}_{k}"] = v
        o, a, r, o1, dn = d["primary_batch"]
        (ao, ao1), (oo, oo1) = d["augmented_obs"], d["original_obs"]
        for tag, t in (("o", o), ("o1", o1), ("ao", ao), ("ao1", ao1), ("oo", oo), ("oo1", oo1)):
            v = t["obs"].cpu().numpy()
            assert np.array_equal(v, np.round(v)) and v.min() >= 0 and v.max() <= 255
            rec[f"m{m}_{tag}"] = v.astype(np.uint8)
        rec[f"m{m}_a"], rec[f"m{m}_r"], rec[f"m{m}_d"] = a.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy()
    rec.update(probes())
    return rec


def run_critic_case(ref, spec):
    """the batch the reference's sample_move_and_augment hands critic_update for the pixel case's buffer (the update itself
    is not recorded: the existing fixtures of that case cover it with its own augmenter).  Two records: s and s'."""
    import case_runner
    import synth
    cfg = synth.CASES[spec["case"]]
    spec = dict(spec, B=cfg["B"])
    k = int(cfg["B"] * spec["aug_mix"])
    seed_all(spec["seed"])
    buf = ref.replay.ReplayBuffer(cfg["cap"])
    s, _a, _r, s1, _d = case_runner._buffers(cfg)
    buf.load_experience(s, _a, _r, s1, _d)
    augs = aug_cases.build(ref.augmentations, spec)
    seq = ref.augmentations.AugmentationSequence(augs)
    d = ref.learning_utils.sample_move_and_augment(buf, cfg["B"], seq, spec["aug_mix"], per=False)
    idx = np.asarray(d["priority_idxs"]).astype(np.int64)
    o, _a, _r, o1, _d = d["primary_batch"]
    (key, v), = o.items()
    recs = []
    for got, rows in ((v.numpy(), s[key]), (o1[key].numpy(), s1[key])):
        assert np.array_equal(got, np.round(got)) and got.min() >= 0 and got.max() <= 255
        assert np.array_equal(got[k:], rows[idx[k:]].astype(np.float32))          # the rows behind the mix: replay rows
        assert not np.array_equal(got[:k], rows[idx[:k]].astype(np.float32))
        recs.append({"idx": idx, "augmented_rows": got[:k].astype(np.uint8)})
    recs[0].update(aug_cases.snapshot(augs, spec))
    return recs


def main(names=None, out=OUT):
    ref = ref_harness.import_reference()
    torch.set_num_threads(1)
    os.makedirs(out, exist_ok=True)
    todo = {**aug_cases.CASES, aug_cases.SMAA["name"]: aug_cases.SMAA, aug_cases.CRITIC["name"]: aug_cases.CRITIC}
    for name in names or sorted(todo):
        if name == aug_cases.SMAA["name"]:
            rec = run_smaa(ref, todo[name])
        elif name == aug_cases.CRITIC["name"]:
            rec, rec_s1 = run_critic_case(ref, todo[name])
            np.savez_compressed(os.path.join(out, f"{aug_cases.CRITIC_FILES[1]}.npz"), **rec_s1)
            assert os.path.getsize(os.path.join(out, f"{aug_cases.CRITIC_FILES[1]}.npz")) <= MAX_BYTES
        else:
            rec = run_case(ref, name, todo[name])
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
