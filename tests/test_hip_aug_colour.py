"""GPU: ColorJitterAug and NetworkRandomizationAug (csrc/ssac_aug_colour.hip: ssac_aug_colour_jitter, ssac_aug_netrand)
against the fp64 restatement of tests/aug_colour_cases.py, with the draws the reference made (tests/golden, written by
tools/gen_aug_colour_golden.py) replayed through the super_sac_amd.rng hooks.

Bound of every comparison with fp64: aug_colour_cases.TOL_FACTOR (4) x the fixture's recorded ref_dev64 -- the distance of
the REFERENCE's fp32 output from the same restatement -- over all elements, on the 0..255 scale.  Outputs of the same
kernel that must agree (uint8 / fp32 source, with / without idx, two launches, stand-alone / sequence) are compared bit
for bit."""
import copy
import math
import random
from itertools import chain

import numpy as np
import pytest
import torch

import aug_colour_cases as cc
import case_runner
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ssa():
    import super_sac_amd
    return super_sac_amd


def _bound(rec):
    return cc.TOL_FACTOR * float(rec["ref_dev64"])


def _replayed(ssa, spec, rec):
    """the case's sequence built from this package's classes, holding the recorded randomisation (drawn through the hooks)"""
    A = ssa.augmentations
    with cc.DrawReplay(ssa.rng, spec, rec, repeat=2):
        seq = A.AugmentationSequence(cc.build(A, spec))
        seq.change_randomization_params()
    return seq


def _orders(spec, rec, k):
    """the contrast-first masks of batch k, one per ColorJitterAug member"""
    if f"order{k}" not in rec:
        return ()
    return tuple(cc.order_bits(f) for f in np.asarray(rec[f"order{k}"]))


def _sources(img, dtype):
    """(src, idx) without and with a gather: the rows scattered over a larger buffer, found again through idx"""
    t = torch.from_numpy(img).to(DEV).to(dtype)
    B = img.shape[0]
    perm = torch.from_numpy(np.random.RandomState(5).permutation(2 * B + 3)[:B].astype(np.int64))
    big = torch.full((2 * B + 3,) + tuple(img.shape[1:]), 77, dtype=dtype, device=DEV)
    big[perm.to(DEV)] = t
    return [(t, None), (big, perm.to(DEV))]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_kernels_match_the_fp64_restatement(ssa, name):
    """every fixture: s and s' where recorded, uint8 and fp32 sources, with and without idx, n_aug 0 / B/2 / B.
    Every comparison prints its distance before it asserts; the figures of the MI355X are in profiles/aug_chain.md
    ("Distance from the fp64 restatement")."""
    spec, rec = cc.CASES[name], cc.load(name)
    seq = _replayed(ssa, spec, rec)
    passes = seq.device_passes()
    assert passes is not None and seq.device_chain() is None
    B, c, h, w = spec["B"], spec["c"], spec["h"], spec["w"]
    dev = torch.device(DEV)
    full = {}
    for k in range(2 if spec["both"] else 1):
        want = cc.restate(spec, rec, k)
        first = None
        for dtype in (torch.uint8, torch.float32):
            for src, idx in _sources(rec[f"in{k}"], dtype):
                keep = src.clone()
                out = passes.run(src, idx, B, c, h, w, B, dev, _orders(spec, rec, k))
                torch.cuda.synchronize()
                assert torch.equal(src, keep)                      # the source rows are read, never written
                err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
                print(f"{name} s{k} {str(dtype)[6:]} {'idx' if idx is not None else 'plain'}: max |kernel - fp64| {err:.3e}, "
                      f"bound {_bound(rec):.3e}")
                assert err <= _bound(rec)
                if first is None:
                    first = out
                assert torch.equal(_bits(out), _bits(first))      # the same values from either source type, gathered or not
        full[k] = first
    # aug_mix: rows >= n_aug are a plain gather + convert, the rows in front are what the full run gave them
    src, idx = _sources(rec["in0"], torch.uint8)[1]
    plain = torch.from_numpy(rec["in0"].astype(np.float32)).to(DEV)
    for n_aug in (0, B // 2, B):
        out = passes.run(src, idx, B, c, h, w, n_aug, dev, _orders(spec, rec, 0))
        assert torch.equal(_bits(out[n_aug:]), _bits(plain[n_aug:])), n_aug
        assert torch.equal(_bits(out[:n_aug]), _bits(full[0][:n_aug])), n_aug


def test_both_orders_forced_on_the_same_input(ssa):
    """contrast_first = 0, then all ones, on the input of aug_jitter_c9: each against fp64, and the two outputs differ by
    more than the bound -- the flag is what decides"""
    spec, rec = cc.CASES["aug_jitter_c9"], cc.load("aug_jitter_c9")
    aug = _replayed(ssa, spec, rec).aug_list[0]
    B, c, h, w = spec["B"], spec["c"], spec["h"], spec["w"]
    src = torch.from_numpy(rec["in0"]).to(DEV)
    fac = [rec[f"p0_{a}"] for a in cc.JITTER_FACTORS]
    outs = []
    for bits, flags in ((0, [False] * 3), (0xFFFFFFFF, [True] * 3)):
        out = aug.apply(src, None, B, c, h, w, B, torch.empty(B, c, h, w, device=DEV), bits).cpu().numpy().astype(np.float64)
        err = float(np.abs(out - cc.jitter64(rec["in0"], fac, flags)).max())
        print(f"order bits {bits:#x}: max |kernel - fp64| {err:.3e}, bound {_bound(rec):.3e}")
        assert err <= _bound(rec)
        outs.append(out)
    gap = float(np.abs(outs[0] - outs[1]).max())
    print(f"max distance between the two orders {gap:.3e}")
    assert gap > _bound(rec)


def test_full_size_frames_from_either_source_type(ssa):
    """3 x 84 x 84 planes: an fp32 source stages 85 KB of LDS (above the 64 KB a launch gets without asking), a uint8 source
    21 KB; both give the same bits.  No fixture has this shape, so the comparison with fp64 uses the largest bound of the
    jitter fixtures: the reference's own distance from fp64 does not grow with the plane (the issue measured 1.1e-4 .. 1.9e-4
    up to 3 x 3 x 84 x 84), and a plane mean of 7056 values adds ~1e-5 on the 0..255 scale."""
    A = ssa.augmentations
    B, c, h, w = 2, 6, 84, 84
    img = cc.images(11, B, c, h, w)
    torch.manual_seed(5)
    bound = max(_bound(cc.load(n)) for n in cc.JITTER_CASES)
    jit, net = A.ColorJitterAug(B), A.NetworkRandomizationAug(B)
    fac = [getattr(jit, a).numpy() for a in cc.JITTER_FACTORS]
    got = {}
    for dtype in (torch.uint8, torch.float32):
        src = torch.from_numpy(img).to(DEV).to(dtype)
        got[dtype] = (jit.apply(src, None, B, c, h, w, B, torch.empty(B, c, h, w, device=DEV), 0b01),
                      net.apply(src, None, B, c, h, w, B, torch.empty(B, c, h, w, device=DEV)))
    for a, b in zip(got[torch.uint8], got[torch.float32]):
        assert torch.equal(_bits(a), _bits(b))
    err = float(np.abs(got[torch.uint8][0].cpu().numpy().astype(np.float64) - cc.jitter64(img, fac, [True, False])).max())
    print(f"84 x 84 jitter: max |kernel - fp64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # network randomisation from the fp32 source (the 85 KB staging): the largest bound of its fixtures, for the same reason
    nbound = max(_bound(cc.load(n)) for n in cc.CASES if n not in cc.JITTER_CASES)
    nerr = float(np.abs(got[torch.float32][1].cpu().numpy().astype(np.float64)
                        - cc.netrand64(img, net.conv.weight.detach().numpy())).max())
    print(f"84 x 84 netrand: max |kernel - fp64| {nerr:.3e}, bound {nbound:.3e}")
    assert nerr <= nbound


@pytest.mark.parametrize("name", ["aug_jitter_c3", "aug_netrand_c3"])
def test_launches_are_bit_equal_and_standalone_equals_the_sequence(ssa, name):
    """two launches on the same input give the same bits (fixed-order reduction, no atomics); aug(imgs) on a device tensor ==
    the one-member sequence, bit for bit, with the same recorded draws; the input is left alone"""
    spec, rec = cc.CASES[name], cc.load(name)
    seq = _replayed(ssa, spec, rec)
    aug = seq.aug_list[0]
    B, c, h, w = spec["B"], spec["c"], spec["h"], spec["w"]
    imgs = torch.from_numpy(rec["in0"]).to(DEV).float()
    keep = imgs.clone()
    dev = torch.device(DEV)
    one = seq.device_passes().run(imgs, None, B, c, h, w, B, dev, _orders(spec, rec, 0))
    two = seq.device_passes().run(imgs, None, B, c, h, w, B, dev, _orders(spec, rec, 0))
    assert torch.equal(_bits(one), _bits(two))
    with cc.DrawReplay(ssa.rng, spec, rec, batches=(0,)) as rp:
        alone = aug(imgs)
        assert len(rp.calls) == (c // 3 if name == "aug_jitter_c3" else 0)
    assert alone.dtype == torch.float32 and alone.data_ptr() != imgs.data_ptr()
    assert torch.equal(_bits(alone), _bits(one)) and torch.equal(imgs, keep)
    # and through the sequence's own call: one randomisation for both batches, the orders of s and s' drawn up front
    with cc.DrawReplay(ssa.rng, spec, rec, batches=(0, 1)):
        a, a1 = seq({"obs": imgs}, {"obs": torch.from_numpy(rec["in1"]).to(DEV).float()})
    assert torch.equal(_bits(a["obs"]), _bits(one)) and torch.equal(imgs, keep)
    err = float(np.abs(a1["obs"].cpu().numpy().astype(np.float64) - cc.restate(spec, rec, 1)).max())
    assert err <= _bound(rec)


def _seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def test_sample_move_and_augment_follows_the_reference(ssa):
    """the reference's sample_move_and_augment with [ColorJitterAug, TranslateAug] on uint8 frames, from the case's seed with
    the STOCK hooks: the indices, factors, translations and order flags the reference drew, the primary batch at aug_mix
    0 / 0.5 / 1 (augmented rows against fp64, the rows behind the mix exactly), the invariance pair from the same flags, and
    the generators end where the reference's did"""
    spec, rec = cc.SMAA, cc.load(cc.SMAA["name"])
    A, lu = ssa.augmentations, ssa.learning_utils
    s, a, r, s1, d = cc.smaa_transitions(spec)
    _seed_all(spec["seed"])
    buf = ssa.replay.ReplayBuffer(spec["rows"], device=torch.device(DEV))
    buf.load_experience(s, a, r, s1, d)
    seq = A.AugmentationSequence(cc.build(A, spec))
    B = spec["B"]
    for m, mix in enumerate(spec["mixes"]):
        sub = {k[3:]: v for k, v in rec.items() if k.startswith(f"m{m}_")}
        flags = []
        stock = ssa.rng.draw_jitter_order
        ssa.rng.draw_jitter_order = lambda b, p: (flags.append(stock(b, p)), flags[-1])[1]
        try:
            dct = lu.sample_move_and_augment(buf, B, seq, mix, per=False, _invariance=True)
        finally:
            ssa.rng.draw_jitter_order = stock
        assert np.array_equal(np.asarray(dct["priority_idxs"]), sub["idx"])
        for k, v in cc.snapshot(seq.aug_list, spec).items():
            assert np.array_equal(v, sub[k]), k
        assert flags == [bool(f) for f in np.concatenate([sub["order0"].reshape(-1), sub["order1"].reshape(-1)])]
        o, a_, r_, o1, dn = dct["primary_batch"]
        k_aug = int(B * mix)
        for k, (got, rows) in enumerate(((o["obs"], s["obs"]), (o1["obs"], s1["obs"]))):
            got = got.cpu().numpy()
            want = cc.restate(spec, sub, k, img=rows[sub["idx"]])
            assert np.array_equal(got[k_aug:], rows[sub["idx"]][k_aug:].astype(np.float32)), mix
            err = float(np.abs(got[:k_aug].astype(np.float64) - want[:k_aug]).max()) if k_aug else 0.0
            print(f"aug_mix {mix} s{k}: max |kernel - fp64| {err:.3e}, bound {_bound(rec):.3e}")
            assert err <= _bound(rec)
        assert np.array_equal(a_.cpu().numpy(), sub["a"]) and np.array_equal(r_.cpu().numpy(), sub["r"])
        assert np.array_equal(dn.cpu().numpy(), sub["d"])
        # the invariance pair: every row augmented / no row augmented, under the flags of (s, key) -- nothing more was drawn
        (ao, _), (oo, _) = dct["augmented_obs"], dct["original_obs"]
        want = cc.restate(spec, sub, 0, img=s["obs"][sub["idx"]])
        assert float(np.abs(ao["obs"].cpu().numpy().astype(np.float64) - want).max()) <= _bound(rec)
        assert np.array_equal(oo["obs"].cpu().numpy(), s["obs"][sub["idx"]].astype(np.float32))
    probes = {"probe_torch": torch.randint(1 << 30, (4,)).numpy(), "probe_numpy": np.random.randint(1 << 30, size=4),
              "probe_python": np.float64(random.random())}
    for k, v in probes.items():
        assert np.array_equal(v, rec[k]), k


class _ForeignSequence:
    def __init__(self, aug_list):
        self.aug_list, self.keys = aug_list, None


def test_reference_shaped_colour_sequence_is_adopted_by_critic_update(ssa):
    """[ColorJitterAug, TranslateAug] as stand-ins that carry the reference classes' names and state (the jitter a real
    torch.nn.Module, as the reference's is), handed to one critic_update of the drqv2_pixels case (9 x 84 x 84 uint8 frames):
    adopted in place on first contact, the update runs and its logs are finite"""
    cfg = synth.CASES["drqv2_pixels"]
    A = ssa.augmentations
    B = cfg["B"]
    jit = type("ColorJitterAug", (torch.nn.Module,), {})()
    for k, v in dict(batch_size=B, brightness=[0.6, 1.4], contrast=[0.6, 1.4], saturation=[0.6, 1.4], hue=[-0.5, 0.5], prob=1.0,
                     stack_size=1, factor_contrast=torch.ones(B), factor_hue=torch.zeros(B), factor_brightness=torch.ones(B),
                     factor_saturate=torch.ones(B)).items():
        setattr(jit, k, v)
    tr = type("TranslateAug", (), {})()
    tr.batch_size, tr.translate_max = B, 4
    tr.translation, tr.random_color = torch.zeros(B, 2, dtype=torch.int32), torch.zeros(B, 3, 1, 1)
    seq = _ForeignSequence([jit, tr])
    dev = torch.device(DEV)
    buf = ssa.replay.ReplayBuffer(cfg["cap"], device=dev)
    buf.load_experience(*case_runner._buffers(cfg))
    agent = case_runner.build_engine_agent(cfg, dev)
    target = copy.deepcopy(agent)
    copt = torch.optim.Adam(chain(*(c.parameters() for c in agent.critics)), lr=cfg["lr"], betas=(0.9, 0.999))
    eopt = torch.optim.Adam(agent.encoder.parameters(), lr=cfg["pixels"]["enc_lr"], betas=(0.9, 0.999))
    las = [torch.Tensor([math.log(1e-15)]).to(dev).requires_grad_()]
    _seed_all(21)
    logs, dicts = ssa.learning.critic_update(
        buffer=buf, agent=agent, target_agent=target, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=las,
        batch_size=B, gamma=cfg["gamma"], critic_clip=cfg["clip"], encoder_clip=cfg["clip"],
        target_critic_ensemble_n=cfg["n"], weighted_bellman_temp=cfg["temp"], weight_type=cfg["weight_type"],
        pop=cfg["pop"], augmenter=seq, encoder_lambda=0, aug_mix=0.5, discrete=False, random_process=None, noise_clip=None,
        per=False, update_priorities=False, dr3_coeff=0.0)
    torch.cuda.synchronize()
    assert type(seq) is A.AugmentationSequence and [type(m) for m in seq.aug_list] == [A.ColorJitterAug, A.TranslateAug]
    assert [type(p) for p in seq.device_passes().passes] == [A.ColorJitterAug, A._ChainPlan]
    assert logs and all(math.isfinite(float(x)) for x in logs.values()), logs
    o = dicts[0]["primary_batch"][0]
    (key, v), = o.items()
    assert v.shape == (B, 9, 84, 84) and bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 and float(v.max()) <= 255.0


def test_host_refusals_text_for_text(ssa):
    """each entry point with ONE defect: a non-zero status and the exact ssac_last_error(); every refusal returns before any
    HIP call, so nothing is launched"""
    lib = ssa._lib.lib
    src = torch.zeros(2 * 99 * 4, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(2 * 99 * 4, dtype=torch.float32, device=DEV)
    par = torch.zeros(81, dtype=torch.float32, device=DEV)
    S, D, P = src.data_ptr(), dst.data_ptr(), par.data_ptr()

    def jitter(src=S, dtype=1, c=3, h=2, w=2, par=P, dst=D):
        return lib.ssac_aug_colour_jitter(src, dtype, 0, 2, c, h, w, par, 0, 2, dst, 0)

    def netrand(src=S, dtype=1, c=3, h=2, w=2, par=P, dst=D):
        return lib.ssac_aug_netrand(src, dtype, 0, 2, c, h, w, par, 2, dst, 0)
    cases = [(dict(c=99), "more than SSAC_AUG_COLOUR_MAX_GROUPS (32) groups of three channels"),
             (dict(par=0), "bad arguments"),
             (dict(src=D, dtype=0), "dst must not alias src"),
             (dict(dtype=2), "unsupported src_dtype"),
             (dict(dtype=0, h=100, w=100), "three image planes do not fit the LDS staging (SSAC_AUG_COLOUR_LDS_BYTES, 96 KB)")]
    for fn, who in ((jitter, "ssac_aug_colour_jitter"), (netrand, "ssac_aug_netrand")):
        for kw, text in cases:
            assert fn(**kw) != 0, (who, kw)
            assert lib.ssac_last_error().decode() == f"{who}: {text}", (who, kw)
        assert fn() == 0                                   # the same call without a defect is accepted
    torch.cuda.synchronize()
