"""CPU: the host side of ColorJitterAug and NetworkRandomizationAug -- the fp64 restatement against the recorded reference
outputs, the reference's draw order (per randomisation and per application), adoption of reference-shaped torch.nn.Module
objects, the refusals, and that sequences without the two classes build what they built before.  No GPU, no reference
tree: tests/golden only."""
import random

import numpy as np
import pytest
import torch

import aug_cases
import aug_colour_cases as cc


def _ssa():
    import super_sac_amd as ssa
    return ssa


def _seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _probes():
    return {"probe_torch": torch.randint(1 << 30, (4,)).numpy(), "probe_numpy": np.random.randint(1 << 30, size=4),
            "probe_python": np.float64(random.random())}


# ------------------------------------------------------------------------------------------ fixtures and restatement
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_restatement_agrees_with_the_recorded_reference(name):
    """the fixture and the fp64 restatement belong together: every element within the recorded ref_dev64 (recomputed here,
    so a fixture cannot carry a figure its own data does not give)"""
    spec, rec = cc.CASES[name], cc.load(name)
    dev = 0.0
    for k in range(2 if spec["both"] else 1):
        assert rec[f"out{k}"].dtype == np.float32 and rec[f"in{k}"].dtype == np.uint8
        dev = max(dev, float(np.abs(rec[f"out{k}"].astype(np.float64) - cc.restate(spec, rec, k)).max()))
    print(f"{name}: ref_dev64 recorded {float(rec['ref_dev64']):.3e}, recomputed {dev:.3e}")
    assert dev <= float(rec["ref_dev64"]) * (1 + 1e-9) + 1e-12
    assert 0.0 < float(rec["ref_dev64"]) < 1e-3
    if name in cc.JITTER_CASES and spec["members"][0][0] == "ColorJitterAug":
        assert cc.planted_present(rec["in0"])


def test_smaa_restatement_agrees_with_the_recorded_reference():
    spec, rec = cc.SMAA, cc.load(cc.SMAA["name"])
    s, _a, _r, s1, _d = cc.smaa_transitions(spec)
    dev = 0.0
    for m, mix in enumerate(spec["mixes"]):
        sub = {k[3:]: v for k, v in rec.items() if k.startswith(f"m{m}_")}
        k_aug = int(spec["B"] * mix)
        for k, (tag, rows) in enumerate((("o", s["obs"]), ("o1", s1["obs"]))):
            want = cc.restate(spec, sub, k, img=rows[sub["idx"]])
            assert np.array_equal(sub[tag][k_aug:], rows[sub["idx"]][k_aug:].astype(np.float32))
            if k_aug:
                dev = max(dev, float(np.abs(sub[tag][:k_aug].astype(np.float64) - want[:k_aug]).max()))
    assert dev <= float(rec["ref_dev64"]) * (1 + 1e-9) and float(rec["ref_dev64"]) < 1e-3


def test_both_orders_are_on_record_and_the_tie_order_shows():
    """what the cases are there for: s and s' of aug_jitter_c3 got different orders under the same factors, both orders
    occur among the groups of aug_jitter_c9, and the restatement's two orders differ by far more than any tolerance.
    The tie order (b over g over r) is visible in the restatement: at r == g > b the g branch gives a hue of
    2 - delta / (delta + eps) sixths, the r branch delta / (delta + eps); the planted r == g > b and g == b > r blocks hold
    every kernel output to the winning branch through the every-element bound."""
    rec = cc.load("aug_jitter_c3")
    assert rec["order0"].shape == (1, 1) and bool(rec["order0"][0, 0]) != bool(rec["order1"][0, 0])
    o9 = cc.load("aug_jitter_c9")["order0"]
    assert o9.shape == (1, 3) and o9.any() and not o9.all()
    fac = [rec[f"p0_{a}"] for a in cc.JITTER_FACTORS]
    a, b = cc.jitter64(rec["in0"], fac, [True]), cc.jitter64(rec["in0"], fac, [False])
    assert np.abs(a - b).max() > 1.0
    # hue of the restatement for one tie pixel, read back through a pure hue shift of 0: green channel = c exactly on the g
    # branch's side of 60 degrees (hue >= 60: r' = x, g' = c), which the r branch (hue < 60: r' = c, g' = x) would swap
    one, zero = np.ones(1), np.zeros(1)
    px = np.array([200, 200, 50], np.float64).reshape(1, 3, 1, 1) / 255.0
    back = cc.hsv_block64(px, zero, one, one)[0, :, 0, 0]
    assert back[1] == px[0, 1, 0, 0] and back[0] < back[1] and back[1] - back[0] < 1e-6
    px = np.array([40, 180, 180], np.float64).reshape(1, 3, 1, 1) / 255.0          # g == b > r: the b branch, hue >= 180
    back = cc.hsv_block64(px, zero, one, one)[0, :, 0, 0]
    assert back[2] == px[0, 2, 0, 0] and back[1] < back[2] and back[2] - back[1] < 1e-6


# ------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("name", ["aug_jitter_c3", "aug_netrand_c3"])
def test_stock_hooks_follow_the_reference(name):
    """construction, one randomisation of the sequence and the application draws of s and s' from the case's seed: the
    recorded parameters and order flags, and the torch, numpy and Python generators end where the reference's did"""
    ssa = _ssa()
    A = ssa.augmentations
    spec, rec = cc.CASES[name], cc.load(name)
    _seed_all(int(rec["seed"]))
    seq = A.AugmentationSequence(cc.build(A, spec), keys=["obs"])
    seq.change_randomization_params()
    orders = seq.draw_orders({"obs": spec["c"]}, {"obs": spec["c"]})
    have = cc.snapshot(seq.aug_list, spec)
    for k, v in have.items():
        assert v.dtype == rec[k].dtype and np.array_equal(v, rec[k]), k
    if name == "aug_jitter_c3":
        assert [o["obs"] for o in orders] == [(cc.order_bits(rec["order0"][0]),), (cc.order_bits(rec["order1"][0]),)]
    else:
        assert orders is None
    pr = _probes()
    for k, v in pr.items():
        assert np.array_equal(v, rec[k]), k


def test_constructor_defaults_repr_and_state_names():
    A = _ssa().augmentations
    j = A.ColorJitterAug(5)
    assert repr(j) == "ColorJitter" and j.batch_size == 5 and j.prob == 1.0 and j.stack_size == 1
    assert j.contrast == [0.6, 1.4] and j.brightness == [0.6, 1.4] and j.saturation == [0.6, 1.4] and j.hue == [-0.5, 0.5]
    for a in cc.JITTER_FACTORS:
        f = getattr(j, a)
        assert f.shape == (5,) and f.dtype == torch.float32
    assert A.ColorJitterAug(3, 0.2, (0.9, 1.1), saturation=0.1, hue=(-0.1, 0.2), unused=1).contrast == (0.9, 1.1)
    n = A.NetworkRandomizationAug(5)
    assert isinstance(n.conv, torch.nn.Conv2d) and n.conv.weight.shape == (3, 3, 3, 3) and n.conv.bias is None
    assert n.conv.padding == (1, 1) and not hasattr(n, "batch_size")
    for aug in (j, n):
        seq = A.AugmentationSequence([aug, A.IdentityAug(5)])
        assert seq.device_passes() is not None and seq.device_passes().passes == [aug]
        assert seq.device_chain() is None and seq.single_shift() is None and not seq.is_identity()


class _CallLog:
    """records the draw_jitter_order calls (the stock hook still draws)"""

    def __init__(self, rng_mod):
        self.rng, self.calls = rng_mod, []

    def __enter__(self):
        self.stock = self.rng.draw_jitter_order

        def hook(batch_size, prob):
            flag = self.stock(batch_size, prob)
            self.calls.append(flag)
            return flag
        self.rng.draw_jitter_order = hook
        return self

    def __exit__(self, *exc):
        self.rng.draw_jitter_order = self.stock


def test_application_draws_are_consumed_batch_major():
    """a two-image-key observation through the draw-only part of __call__ (draw_orders) and of sample_move_and_augment
    (learning_utils.draw_augmentation_orders): s then s', key in AugmentationSequence.keys order, member, frame group; a key
    outside `keys` draws nothing; handing a pass its flags again (the invariance re-runs) draws nothing"""
    ssa = _ssa()
    A = ssa.augmentations
    B = 4
    _seed_all(7)
    j0, j1 = A.ColorJitterAug(B), A.ColorJitterAug(B)
    seq = A.AugmentationSequence([j0, A.TranslateAug(B), j1], keys=["pix", "cam"])
    chan = {"cam": 6, "other": 3, "pix": 9}      # (storage order differs from the sequence's key order)
    for draw in (lambda: seq.draw_orders(chan, chan), lambda: ssa.learning_utils.draw_augmentation_orders(seq, chan)):
        with _CallLog(ssa.rng) as log:
            orders = draw()
        # per batch: pix (3 groups) x 2 members, then cam (2 groups) x 2 members
        assert len(log.calls) == 2 * (3 * 2 + 2 * 2)
        it = iter(log.calls)
        for batch in orders:
            for key, groups in (("pix", 3), ("cam", 2)):
                for member in range(2):
                    want = sum(1 << g for g in range(groups) if next(it))
                    assert batch[key][member] == want
            assert batch["other"] == (0, 0)
    # the stock draw itself: numpy's row selection is consumed even at prob 1, then one Python uniform
    _seed_all(3)
    flag = ssa.rng.draw_jitter_order(B, 1.0)
    after = _probes()
    _seed_all(3)
    np.random.choice([True, False], B, p=[1.0, 0.0])
    assert flag == (random.uniform(0, 1) >= 0.5)
    for k, v in _probes().items():
        assert np.array_equal(v, after[k])
    # a sequence without a ColorJitterAug draws nothing at application time
    with _CallLog(ssa.rng) as log:
        assert A.AugmentationSequence([A.TranslateAug(B), A.NetworkRandomizationAug(B)], keys=["pix"]).draw_orders(chan) is None
    assert not log.calls


# ------------------------------------------------------------------------------------------ adoption
class _ForeignSequence:
    def __init__(self, aug_list):
        self.aug_list, self.keys = aug_list, None


def _module_stand_in(name, **state):
    """a real torch.nn.Module instance that carries the reference class's NAME and state, nothing of this package"""
    obj = type(name, (torch.nn.Module,), {})()
    for k, v in state.items():
        setattr(obj, k, v)
    return obj


def _jitter_state(B, **over):
    st = dict(batch_size=B, brightness=[0.6, 1.4], contrast=[0.6, 1.4], saturation=[0.6, 1.4], hue=[-0.5, 0.5], prob=1.0,
              stack_size=1, factor_contrast=torch.linspace(0.7, 1.3, B), factor_hue=torch.linspace(-0.4, 0.4, B),
              factor_brightness=torch.linspace(0.8, 1.2, B), factor_saturate=torch.linspace(0.9, 1.1, B),
              _device=torch.device("cpu"))
    st.update(over)
    return st


def test_adoption_of_reference_shaped_modules():
    ssa = _ssa()
    A = ssa.augmentations
    B = 4
    jit = _module_stand_in("ColorJitterAug", **_jitter_state(B))
    conv = torch.nn.Conv2d(3, 3, kernel_size=3, bias=False, padding=1)
    net = _module_stand_in("NetworkRandomizationAug", conv=conv, _device="cpu")      # (no batch_size, as the reference's)
    assert not hasattr(net, "batch_size") and "conv" not in net.__dict__
    seq = _ForeignSequence([jit, net])
    gen = (torch.get_rng_state(), np.random.get_state()[1].copy(), random.getstate())
    assert ssa.adopt_augmenter(seq) is seq
    assert torch.equal(torch.get_rng_state(), gen[0]) and np.array_equal(np.random.get_state()[1], gen[1])
    assert random.getstate() == gen[2]                                   # no draw consumed
    assert type(seq) is A.AugmentationSequence and type(jit) is A.ColorJitterAug and type(net) is A.NetworkRandomizationAug
    assert repr(jit) == "ColorJitter" and net.conv is conv
    # the state they held is the state the kernels get
    want = torch.stack([torch.linspace(0.7, 1.3, B), torch.linspace(-0.4, 0.4, B), torch.linspace(0.8, 1.2, B),
                        torch.linspace(0.9, 1.1, B)], dim=1)
    assert torch.equal(jit._host_params(), want)
    assert torch.equal(net._host_params(), conv.weight.detach().reshape(81))
    assert [type(p) for p in seq.device_passes().passes] == [A.ColorJitterAug, A.NetworkRandomizationAug]
    assert ssa.adopt_augmenter(seq) is seq                               # idempotent
    # the next randomisation is drawn by this package's classes, on the same generators
    torch.manual_seed(3)
    jit.change_randomization_params()
    net.change_randomization_params()
    torch.manual_seed(3)
    again, again_net = A.ColorJitterAug(B), A.NetworkRandomizationAug(B)
    for a in cc.JITTER_FACTORS:
        assert torch.equal(getattr(jit, a), getattr(again, a)), a
    assert torch.equal(net.conv.weight, again_net.conv.weight)


@pytest.mark.parametrize("over,why", [(dict(stack_size=2), "stack_size = 2"), (dict(prob=0.5), "p_rand = 0.5"),
                                      (dict(brightness=None), "brightness is a zero range")])
def test_what_the_reference_cannot_run_is_refused(over, why):
    """at adoption and at construction, naming the reference's own failure"""
    ssa = _ssa()
    jit = _module_stand_in("ColorJitterAug", **_jitter_state(4, **over))
    with pytest.raises(NotImplementedError, match="no HIP path") as e:
        ssa.adopt_augmenter(_ForeignSequence([jit]))
    assert why in str(e.value) and "reference's own class raises" in str(e.value)
    assert type(jit).__module__ != ssa.augmentations.__name__            # nothing was swapped
    kw = {"stack_size": dict(stack_size=2), "prob": dict(p_rand=0.5), "brightness": dict(brightness=0)}[next(iter(over))]
    with pytest.raises(NotImplementedError, match="no HIP path") as e:
        ssa.augmentations.ColorJitterAug(4, **kw)
    assert why in str(e.value)


def test_names_alone_are_still_refused_with_true_reasons():
    ssa = _ssa()
    for cls, needles in (("ColorJitterAug", ("draws inside forward", "does not carry its state", "factor_contrast")),
                         ("NetworkRandomizationAug", ("does not carry the convolution", "missing ['conv']"))):
        bare = type(cls, (), {})()
        bare.batch_size = 4
        with pytest.raises(NotImplementedError, match="no HIP path") as e:
            ssa.adopt_augmenter(_ForeignSequence([bare]))
        for n in needles:
            assert n in str(e.value), (cls, n)
        assert "not built yet" not in str(e.value)


# ------------------------------------------------------------------------------------------ nothing else changed
def test_sequences_without_the_new_classes_build_what_they_built():
    """same pass types and the same host table as the chain fixtures pin (tests/test_aug_cpu.py holds the tables to the
    reference's outputs); the DrQ family alone still has no pass plan"""
    ssa = _ssa()
    A = ssa.augmentations
    for name in ("aug_chain_tcf", "aug_mixed_drqv2"):
        spec, rec = aug_cases.CASES[name], aug_cases.load(name)
        with aug_cases.DrawReplay(ssa.rng, spec, rec, repeat=2):
            seq = A.AugmentationSequence(aug_cases.build(A, spec))
            seq.change_randomization_params()
        passes = seq.device_passes().passes
        if name == "aug_chain_tcf":
            assert [type(p) for p in passes] == [A._ChainPlan] and seq.device_chain() is passes[0]
            want = aug_cases.walk_table(passes[0].host_table(), rec["in0"])
            assert np.array_equal(want, rec["out0"].astype(np.float32))
        else:
            assert [type(p) for p in passes] == [A._ChainPlan, A.Drqv2Aug, A._ChainPlan] and seq.device_chain() is None
        assert seq.draw_orders({"obs": spec["c"]}) is None
    drq = A.AugmentationSequence([A.Drqv2Aug(4)])
    assert drq.device_passes() is None and drq.single_shift() is drq.aug_list[0]
    assert A.AugmentationSequence([A.IdentityAug(4)]).device_passes() is None
