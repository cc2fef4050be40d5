"""Time ssac_aug_chain, ssac_aug_colour_jitter and ssac_aug_netrand against the DrQv2 mode of ssac_drq_shift on the MI355X
(profiles/aug_chain.md).

    python tools/bench_aug.py [--batch 512] [--regions 15] [--launches 50]

Shape: B x 9 x 84 x 84, uint8 replay rows read through idx, fp32 out -- what one observation batch of the DMC pixel
configuration moves.  The kernels alternate region by region in one process (warm clocks, same machine state): a single
TranslateAug, the four-member chain [Rotate, Window, Gamma, Cutout] (also without its gamma, and the gamma alone), ColorJitterAug
alone (both orders among its three frame groups), NetworkRandomizationAug alone, the three passes of [Translate, ColorJitter,
HorizontalFlip] (the figure of that row is all three launches and its two fp32 temporaries), and Drqv2Aug.  A region is `launches` back-to-back
launches between two device events; the figure of a kernel is the median over its regions, with min and max as the spread.
Bytes per launch = B * 9 * 84 * 84 * (1 read + 4 written).
"""
import argparse
import json
import statistics

import torch

import super_sac_amd as ssa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--regions", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    A, dev = ssa.augmentations, torch.device("cuda")
    B, c, h = args.batch, 9, 84
    torch.manual_seed(0)
    rows = 4 * B
    src = torch.randint(0, 256, (rows, c, h, h), dtype=torch.uint8, device=dev)
    idx = torch.randint(rows, (B,), device=dev)
    out = torch.empty(B, c, h, h, device=dev)
    rot = A.RotateAug(B)
    rot.random_inds = torch.arange(B) % 4          # (a quarter of the rows each: untouched, 180, 270, untouched)
    plans = {
        "translate": A._ChainPlan([A.TranslateAug(B)]),
        "chain4": A._ChainPlan([rot, A.WindowAug(B), A.GammaAug(B), A.CutoutAug(B)]),
        # where chain4's time goes: the same chain without its gamma, and the gamma alone
        "chain3_no_gamma": A._ChainPlan([rot, A.WindowAug(B), A.CutoutAug(B)]),
        "gamma": A._ChainPlan([A.GammaAug(B)]),
    }
    shift = A.Drqv2Aug(B)
    runs = {name: (lambda p=p: p.apply(src, idx, B, c, h, h, B, out)) for name, p in plans.items()}
    jitter, netrand = A.ColorJitterAug(B), A.NetworkRandomizationAug(B)
    mixed = A._DevicePasses([A.TranslateAug(B), A.ColorJitterAug(B), A.HorizontalFlipAug(B)])
    runs["colour_jitter"] = lambda: jitter.apply(src, idx, B, c, h, h, B, out, 0b101)
    runs["netrand"] = lambda: netrand.apply(src, idx, B, c, h, h, B, out)
    runs["translate_jitter_hflip"] = lambda: mixed.run(src, idx, B, c, h, h, B, dev, (0b101,))
    runs["drqv2_shift"] = lambda: shift.apply(src, idx, B, c, h, B, out)
    for fn in runs.values():                        # warm-up: code objects, table uploads, clocks
        for _ in range(200):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(args.regions):
        for name, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)   # us per launch
    nbytes = B * c * h * h * 5
    res = {"batch": B, "shape": [c, h, h], "bytes_per_launch": nbytes, "regions": args.regions, "launches": args.launches}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                     "gb_per_s": round(nbytes / med / 1e3, 1)}
    for name in [n for n in runs if n != "drqv2_shift"]:
        res[name]["ratio_to_translate"] = round(res[name]["median_us"] / res["translate"]["median_us"], 3)
        res[name]["ratio_to_drqv2_shift"] = round(res[name]["median_us"] / res["drqv2_shift"]["median_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
