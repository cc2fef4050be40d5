"""GPU: the chained augmentations (csrc/ssac_aug.hip: ssac_aug_chain) against the reference's recorded outputs
(tests/golden/aug_*.npz, written by tools/gen_aug_golden.py), draws replayed through the super_sac_amd.rng hooks."""
import copy
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import aug_cases
import case_runner
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _replayed(ssa, spec, rec):
    """the case's sequence built from this package's classes, holding the recorded randomisation (drawn through the hooks)"""
    A = ssa.augmentations
    with aug_cases.DrawReplay(ssa.rng, spec, rec, repeat=2):
        seq = A.AugmentationSequence(aug_cases.build(A, spec))
        seq.change_randomization_params()
    return seq


def _ulps(a, b):
    """distance in units of the last place between two positive finite fp32 arrays"""
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def _check_gamma(got, want, who):
    """rtol 1e-6 on the non-zero reference values, exact where the reference is 0 or 255 (the bound: bit-identical inputs,
    torch's CPU pow within 1 ulp, the fp64 power rounded once within 0.5 ulp, one more fp32 rounding on each side:
    <= ~2.5 ulp ~ 3e-7 relative)"""
    edge = (want == 0) | (want == 255)
    mid = ~edge
    ulp = int(_ulps(got[mid], want[mid]).max()) if mid.any() else 0
    rel = float((np.abs(got[mid] - want[mid]) / want[mid]).max()) if mid.any() else 0.0
    print(f"{who}: gamma max ulp distance {ulp}, max relative error {rel:.3e}, "
          f"{int(edge.sum())} of {want.size} values at 0 / 255")
    assert np.array_equal(got[edge], want[edge])
    assert np.allclose(got[mid], want[mid], rtol=1e-6, atol=0.0)
    return ulp


def _sources(img, dtype):
    """(src, idx) without and with a gather: the rows scattered over a larger buffer, found again through idx"""
    t = torch.from_numpy(img).to(DEV).to(dtype)
    B = img.shape[0]
    perm = torch.from_numpy(np.random.RandomState(5).permutation(2 * B + 3)[:B].astype(np.int64))
    big = torch.full((2 * B + 3,) + tuple(img.shape[1:]), 77, dtype=dtype, device=DEV)
    big[perm.to(DEV)] = t
    return [(t, None), (big, perm.to(DEV))]


CHAIN_ONLY = sorted(n for n, s in aug_cases.CASES.items() if not any(c == "Drqv2Aug" for c, _ in s["members"]))


@pytest.mark.parametrize("name", CHAIN_ONLY)
def test_chain_kernel_matches_the_reference(ssa, name):
    """every class alone (9 and 3 channels, s and s' under one randomisation) and the chains of 3-5 members: one
    ssac_aug_chain launch, uint8 and fp32 sources, with and without idx.  np.array_equal for everything that moves or fills
    integer-valued data; Gamma within rtol 1e-6 (exact at 0 and 255).
    Measured on the MI355X (profiles/aug_chain.md): the largest distance of a Gamma output from the reference's is 1 ulp
    (1.1e-7 relative) for GammaAug alone and for the 4-member chain, 2 ulp (2.1e-7 relative) for the chain that applies two
    gammas in a row; uint8 and fp32 sources, with and without idx, give the same figures."""
    spec, rec = aug_cases.CASES[name], aug_cases.load(name)
    seq = _replayed(ssa, spec, rec)
    plan = seq.device_chain()
    assert plan is not None
    B, c, hw = spec["B"], spec["c"], spec["hw"]
    for k in range(2 if spec["both"] else 1):
        want = rec[f"out{k}"].astype(np.float32)
        for dtype in (torch.uint8, torch.float32):
            for src, idx in _sources(rec[f"in{k}"], dtype):
                keep = src.clone()
                out = torch.empty(B, c, hw, hw, device=DEV)
                plan.apply(src, idx, B, c, hw, hw, B, out)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert torch.equal(src, keep)                      # the source rows are read, never written
                who = f"{name} s{k} {str(dtype)[6:]} {'idx' if idx is not None else 'plain'}"
                if aug_cases.is_exact(spec):
                    assert np.array_equal(got, want), who
                else:
                    _check_gamma(got, want, who)
    # aug_mix: rows >= n_aug are a plain gather + convert
    src, idx = _sources(rec["in0"], torch.uint8)[1]
    n_aug = B // 2
    out = torch.empty(B, c, hw, hw, device=DEV)
    plan.apply(src, idx, B, c, hw, hw, n_aug, out)
    got, full = out.cpu().numpy(), rec["out0"].astype(np.float32)
    assert np.array_equal(got[n_aug:], rec["in0"][n_aug:].astype(np.float32))
    if aug_cases.is_exact(spec):
        assert np.array_equal(got[:n_aug], full[:n_aug])
    else:
        _check_gamma(got[:n_aug], full[:n_aug], name + " mix")


@pytest.mark.parametrize("shape", [(5, 3, 21, 30), (4, 6, 30, 21), (3, 3, 7, 9)])
def test_odd_shapes_take_the_scalar_paths(ssa, shape):
    """planes whose size is not a multiple of 16 / 4 bytes and that are not square: the scalar staging loop, the one-pixel
    compute loop and the scalar plain copy.  No fixture has such a shape, so the kernel is compared with the numpy walk of
    the same op table (aug_cases.walk_table, which tests/test_aug_cpu.py holds to the reference's outputs).  Exact without
    Gamma; with Gamma the bound of _check_gamma (walk_table takes the power in fp64 and rounds once, like the kernel)."""
    A = ssa.augmentations
    B, c, h, w = shape
    rs = np.random.RandomState(h * w)
    img = rs.randint(0, 256, shape).astype(np.uint8)
    img[rs.rand(*shape) < 0.1] = 0
    torch.manual_seed(h)
    np.random.seed(w)
    rot = A.RotateAug(B)
    rot.random_inds = torch.tensor([5, 1, 9, 1, 1][:B])          # rows 1 and 3: half turns, which a non-square plane allows
    chains = {"geom": [A.TranslateAug(B, 3), A.HorizontalFlipAug(B), rot, A.VerticalFlipAug(B),
                       A.CutoutColorAug(B, 2, 6, 1, 2), A.CutoutAug(B, 2, 6, 3, 1)],
              "gamma": [A.GammaAug(B), A.LargeTranslateAug(B, 5), A.WindowAug(B), A.GammaAug(B)]}
    for name, members in chains.items():
        if name == "gamma":
            members[2].crop_size = 12                             # (a window that cuts into these small planes)
        plan = A._ChainPlan(members)
        tab = plan.host_table()
        assert (tab[:, :, 0] != A.AUG_NOP).any(axis=1).all() or name == "geom"
        want = aug_cases.walk_table(tab, img)
        for dtype in (torch.uint8, torch.float32):
            for src, idx in _sources(img, dtype):
                for n_aug in (B, B // 2):
                    out = torch.full((B, c, h, w), -1.0, device=DEV)
                    plan.apply(src, idx, B, c, h, w, n_aug, out)
                    got = out.cpu().numpy()
                    assert np.array_equal(got[n_aug:], img[n_aug:].astype(np.float32))
                    if name == "geom":
                        assert np.array_equal(got[:n_aug], want[:n_aug]), (name, dtype, n_aug)
                    else:
                        _check_gamma(got[:n_aug], want[:n_aug], f"odd {shape} {name}")


@pytest.mark.parametrize("m", [0, 2], ids=["mix0", "mix1"])
def test_keys_outside_the_sequence_are_left_alone(ssa, m):
    """AugmentationSequence(keys=[...]): a 4-D key that is not listed is gathered and converted, never augmented -- in the
    primary batch, in augmented_obs and in original_obs, at aug_mix 0 and 1"""
    spec, rec = aug_cases.SMAA, aug_cases.load("aug_smaa")
    mix = spec["mixes"][m]
    A, lu = ssa.augmentations, ssa.learning_utils
    s, a, r, s1, d = aug_cases.smaa_transitions(spec)
    s["other"], s1["other"] = s["obs"][:, :, ::-1].copy(), s1["obs"][:, :, ::-1].copy()
    buf = ssa.replay.ReplayBuffer(spec["rows"], device=torch.device(DEV))
    buf.load_experience(s, a, r, s1, d)
    sub = {k[3:]: v for k, v in rec.items() if k.startswith(f"m{m}_")}
    with aug_cases.DrawReplay(ssa.rng, spec, sub, repeat=2):
        seq = A.AugmentationSequence(aug_cases.build(A, spec), keys=["obs"])
        saved = ssa.rng.draw_indices
        ssa.rng.draw_indices = lambda n, b: torch.from_numpy(sub["idx"].copy())
        try:
            dct = lu.sample_move_and_augment(buf, spec["B"], seq, mix, per=False, _invariance=True)
        finally:
            ssa.rng.draw_indices = saved
    o, _a, _r, o1, _d = dct["primary_batch"]
    (ao, _), (oo, _) = dct["augmented_obs"], dct["original_obs"]
    plain, plain1 = s["other"][sub["idx"]].astype(np.float32), s1["other"][sub["idx"]].astype(np.float32)
    assert np.array_equal(o["obs"].cpu().numpy(), sub["o"].astype(np.float32))
    assert np.array_equal(o["other"].cpu().numpy(), plain) and np.array_equal(o1["other"].cpu().numpy(), plain1)
    assert np.array_equal(ao["other"].cpu().numpy(), plain) and np.array_equal(oo["other"].cpu().numpy(), plain)
    assert np.array_equal(ao["obs"].cpu().numpy(), sub["ao"].astype(np.float32))
    assert np.array_equal(oo["obs"].cpu().numpy(), sub["oo"].astype(np.float32))


def test_mixed_sequence_with_drqv2_matches_the_reference(ssa):
    """[Cutout, Drqv2Aug, HorizontalFlip]: chain pass, ssac_drq_shift pass, chain pass through temporaries.  The bilinear
    DrQv2 shift is not integer-valued; its bound is the one tests/test_hip_kernels.py holds ssac_drq_shift to against the
    reference (4e-3 on the 0..255 scale)."""
    spec, rec = aug_cases.CASES["aug_mixed_drqv2"], aug_cases.load("aug_mixed_drqv2")
    seq = _replayed(ssa, spec, rec)
    assert seq.device_chain() is None
    passes = seq.device_passes()
    B, c, hw = spec["B"], spec["c"], spec["hw"]
    for src, idx in _sources(rec["in0"], torch.uint8) + _sources(rec["in0"], torch.float32):
        got = passes.run(src, idx, B, c, hw, hw, B, torch.device(DEV)).cpu().numpy()
        err = float(np.abs(got - rec["out0"]).max())
        print("mixed drqv2: max abs err", err)
        assert err <= 4e-3
    # through the sequence's own call, on device tensors
    with aug_cases.DrawReplay(ssa.rng, spec, rec):
        out = seq({"obs": torch.from_numpy(rec["in0"]).to(DEV).float()})
    assert float(np.abs(out["obs"].cpu().numpy() - rec["out0"]).max()) <= 4e-3


@pytest.mark.parametrize("cls", aug_cases.CHAIN_CLASSES)
def test_standalone_call_equals_the_single_member_chain(ssa, cls):
    """aug(imgs) on a device tensor == the fused chain with that one member, bit for bit; the input is left alone"""
    name = f"aug_{cls}_c9"
    spec, rec = aug_cases.CASES[name], aug_cases.load(name)
    seq = _replayed(ssa, spec, rec)
    aug = seq.aug_list[0]
    B, c, hw = spec["B"], spec["c"], spec["hw"]
    imgs = torch.from_numpy(rec["in0"]).to(DEV).float()
    keep = imgs.clone()
    alone = aug(imgs)
    fused = torch.empty(B, c, hw, hw, device=DEV)
    seq.device_chain().apply(imgs, None, B, c, hw, hw, B, fused)
    assert alone.dtype == torch.float32 and alone.data_ptr() != imgs.data_ptr()
    assert torch.equal(alone.view(torch.int32), fused.view(torch.int32)) and torch.equal(imgs, keep)
    # and through the sequence's own call: one randomisation for both batches, the inputs left alone
    with aug_cases.DrawReplay(ssa.rng, spec, rec):
        a, a1 = seq({"obs": imgs}, {"obs": imgs})
    assert torch.equal(a["obs"].view(torch.int32), fused.view(torch.int32)) and torch.equal(a1["obs"], a["obs"])
    assert torch.equal(imgs, keep)


def _smaa_buffer(ssa, spec):
    buf = ssa.replay.ReplayBuffer(spec["rows"], device=torch.device(DEV))
    buf.load_experience(*aug_cases.smaa_transitions(spec))
    return buf


@pytest.mark.parametrize("invariance", [False, True])
def test_sample_move_and_augment_matches_the_reference(ssa, invariance):
    """the reference's sample_move_and_augment on a ReplayBuffer of uint8 frames, aug_mix 0 / 0.5 / 1: primary batch,
    augmented and original observations, exact (no Gamma in the sequence)"""
    spec, rec = aug_cases.SMAA, aug_cases.load("aug_smaa")
    A, lu = ssa.augmentations, ssa.learning_utils
    buf = _smaa_buffer(ssa, spec)
    first = {k[3:]: v for k, v in rec.items() if k.startswith("m0_")}
    with aug_cases.DrawReplay(ssa.rng, spec, first):
        seq = A.AugmentationSequence(aug_cases.build(A, spec))
    saved = ssa.rng.draw_indices
    try:
        for m, mix in enumerate(spec["mixes"]):
            sub = {k[len(f"m{m}_"):]: v for k, v in rec.items() if k.startswith(f"m{m}_")}
            ssa.rng.draw_indices = lambda n, b, _i=sub["idx"]: torch.from_numpy(_i.copy())
            with aug_cases.DrawReplay(ssa.rng, spec, sub):
                d = lu.sample_move_and_augment(buf, spec["B"], seq, mix, per=False, _invariance=invariance)
            assert np.array_equal(np.asarray(d["priority_idxs"]), sub["idx"])
            o, a, r, o1, dn = d["primary_batch"]
            assert np.array_equal(o["obs"].cpu().numpy(), sub["o"].astype(np.float32)), mix
            assert np.array_equal(o1["obs"].cpu().numpy(), sub["o1"].astype(np.float32)), mix
            assert np.array_equal(a.cpu().numpy(), sub["a"]) and np.array_equal(r.cpu().numpy(), sub["r"])
            assert np.array_equal(dn.cpu().numpy(), sub["d"])
            if invariance:
                (ao, _), (oo, _) = d["augmented_obs"], d["original_obs"]
                assert np.array_equal(ao["obs"].cpu().numpy(), sub["ao"].astype(np.float32)), mix
                assert np.array_equal(oo["obs"].cpu().numpy(), sub["oo"].astype(np.float32)), mix
                if mix == 1.0:
                    assert ao["obs"] is o["obs"]      # shared where the mix already is one of them
                if mix == 0.0:
                    assert oo["obs"] is o["obs"]
            else:
                assert d["augmented_obs"] is None and d["original_obs"] is None
    finally:
        ssa.rng.draw_indices = saved


class _ForeignSequence:
    def __init__(self, aug_list):
        self.aug_list, self.keys = aug_list, None


def _pixel_update(ssa, aug, idx):
    """one critic_update of synth.CASES["drqv2_pixels"] (9 x 84 x 84 uint8 frames, BigPixelEncoder) with `aug`"""
    cfg = synth.CASES[aug_cases.CRITIC["case"]]
    dev = torch.device(DEV)
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    agent = case_runner.build_engine_agent(cfg, dev)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=cfg["pixels"]["enc_lr"], betas=(0.9, 0.999))
    las = [torch.Tensor([math.log(1e-15)]).to(dev).requires_grad_()]
    saved = ssa.rng.draw_indices
    ssa.rng.draw_indices = lambda n, b: torch.from_numpy(idx.copy())
    try:
        logs, dicts = ssa.learning.critic_update(
            buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
            batch_size=cfg["B"], gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
            target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=cfg["temp"], weight_type=cfg["weight_type"],
            pop=cfg["pop"], augmenter=aug, encoder_lambda=0, aug_mix=aug_cases.CRITIC["aug_mix"], discrete=False,
            random_process=None, noise_clip=None, per=False, update_priorities=False, dr3_coeff=0.0)
    finally:
        ssa.rng.draw_indices = saved
    torch.cuda.synchronize()
    return logs, dicts


def _check_critic_batch(logs, dicts, rec):
    """the whole primary batch, pixel for pixel: the augmented rows against the reference's record, the rows behind the mix
    against the replay rows the recorded indices name"""
    cfg = synth.CASES[aug_cases.CRITIC["case"]]
    k = int(cfg["B"] * aug_cases.CRITIC["aug_mix"])
    s, _a, _r, s1, _d = case_runner._buffers(cfg)
    o, _a, _r, o1, _d = dicts[0]["primary_batch"]
    (key, v), = o.items()
    for got, rows, name in ((v, s[key], aug_cases.CRITIC_FILES[0]), (o1[key], s1[key], aug_cases.CRITIC_FILES[1])):
        got, want = got.cpu().numpy(), aug_cases.load(name)
        assert got.shape == (cfg["B"],) + rows.shape[1:] and want["augmented_rows"].shape[0] == k
        assert np.array_equal(got[:k], want["augmented_rows"].astype(np.float32)), name
        assert np.array_equal(got[k:], rows[want["idx"][k:]].astype(np.float32)), name
    assert logs and all(math.isfinite(float(x)) for x in logs.values()), logs


def test_pixel_critic_update_with_a_three_member_chain(ssa):
    """[Translate, CutoutColor, HorizontalFlip] at aug_mix 0.5 on the drqv2_pixels case: the batch the update trained on is
    the reference's, pixel for pixel (aug_cases.CRITIC), and its losses are finite"""
    spec = dict(aug_cases.CRITIC, B=synth.CASES[aug_cases.CRITIC["case"]]["B"])
    rec = aug_cases.load("aug_critic_update")
    A = ssa.augmentations
    with aug_cases.DrawReplay(ssa.rng, spec, rec, repeat=2):
        seq = A.AugmentationSequence(aug_cases.build(A, spec))
        logs, dicts = _pixel_update(ssa, seq, rec["idx"])
    _check_critic_batch(logs, dicts, rec)


def test_reference_shaped_sequence_is_adopted_by_critic_update(ssa):
    """stand-ins that carry the reference classes' names and state (no class of this package), handed to critic_update: it
    adopts them in place on first contact; the randomisation of the update is drawn by the adopted objects"""
    spec = dict(aug_cases.CRITIC, B=synth.CASES[aug_cases.CRITIC["case"]]["B"])
    rec = aug_cases.load("aug_critic_update")
    A = ssa.augmentations
    B = spec["B"]

    def stand_in(name, bases=(), **state):
        obj = type(name, bases, {})()
        obj.batch_size = B
        for k, v in state.items():
            setattr(obj, k, v)
        return obj
    members = [
        stand_in("TranslateAug", translate_max=4, translation=torch.zeros(B, 2, dtype=torch.int32),
                 random_color=torch.zeros(B, 3, 1, 1)),
        stand_in("CutoutColorAug", box_min=7, box_max=22, pivot_h=12, pivot_w=24, w1=torch.full((B,), 7), h1=torch.full((B,), 7),
                 rand_box=torch.zeros(B, 3, 1, 1)),
        stand_in("HorizontalFlipAug", bases=(type("_FlipAug", (), {}),), p_flip=0.5, dim=3, random_inds=np.zeros(B, bool)),
    ]
    seq = _ForeignSequence(members)
    with aug_cases.DrawReplay(ssa.rng, spec, rec):
        logs, dicts = _pixel_update(ssa, seq, rec["idx"])
    assert type(seq) is A.AugmentationSequence
    assert [type(m) for m in members] == [A.TranslateAug, A.CutoutColorAug, A.HorizontalFlipAug]
    _check_critic_batch(logs, dicts, rec)


def test_resumed_run_draws_the_same_parameters(ssa, tmp_path):
    """nothing of an augmentation needs saving: its randomisation is redrawn before every batch from the host generators,
    which checkpoint.save_training_state / load_training_state carry.  A resumed run draws what the original drew next."""
    A = ssa.augmentations
    cfg = synth.CASES["redq_small"]
    agent = case_runner.build_engine_agent(cfg, torch.device(DEV))
    members = [("TranslateAug", {}), ("CutoutColorAug", {}), ("HorizontalFlipAug", {}), ("RotateAug", {}), ("WindowAug", {}),
               ("GammaAug", {}), ("CutoutAug", {}), ("VerticalFlipAug", {})]
    spec = dict(B=16, members=members)
    torch.manual_seed(11); np.random.seed(11); random.seed(11)
    seq = A.AugmentationSequence(aug_cases.build(A, spec))
    seq.change_randomization_params()
    ssa.checkpoint.save_training_state(str(tmp_path), agent)
    seq.change_randomization_params()
    want = aug_cases.snapshot(seq.aug_list, spec)
    want_table = seq.device_chain().host_table()
    torch.manual_seed(99); np.random.seed(99); random.seed(99)         # the generators move on ...
    resumed = A.AugmentationSequence(aug_cases.build(A, spec))           # ... a fresh process builds its augmenter ...
    ssa.checkpoint.load_training_state(str(tmp_path), agent)            # ... and loads the checkpoint
    resumed.change_randomization_params()
    have = aug_cases.snapshot(resumed.aug_list, spec)
    assert sorted(have) == sorted(want)
    for k in want:
        assert np.array_equal(have[k], want[k]), k
    assert np.array_equal(resumed.device_chain().host_table(), want_table)
