"""CPU: the chained augmentations' host side -- constructors, defaults, __repr__, the reference's draw order, the op table
ssac_aug_chain walks (checked against the reference's outputs through a numpy restatement of the kernel's walk), adoption of
reference-shaped objects, the refusals, install() rebinding.  No GPU, no reference tree: tests/golden only."""
import random
import types

import numpy as np
import pytest
import torch

import aug_cases


def _ssa():
    import super_sac_amd as ssa
    return ssa


DEFAULTS = {
    "CutoutAug": dict(box_min=7, box_max=22, pivot_h=12, pivot_w=24),
    "CutoutColorAug": dict(box_min=7, box_max=22, pivot_h=12, pivot_w=24),
    "TranslateAug": dict(translate_max=4), "LargeTranslateAug": dict(translate_max=8),
    "HorizontalFlipAug": dict(p_flip=0.5, dim=3), "VerticalFlipAug": dict(p_flip=0.5, dim=2),
    "RotateAug": {}, "WindowAug": dict(crop_size=64, crop_max=11), "GammaAug": dict(gamma_mean=1.0, gamma_std=0.45),
}


@pytest.mark.parametrize("cls", aug_cases.CHAIN_CLASSES)
def test_constructor_defaults_and_repr(cls):
    A = _ssa().augmentations
    aug = getattr(A, cls)(5)
    assert aug.batch_size == 5 and repr(aug) == aug_cases.REPR[cls]
    for name, want in DEFAULTS[cls].items():
        assert getattr(aug, name) == want, (cls, name)
    for attr in aug_cases.STATE[cls]:
        assert len(getattr(aug, attr)) == 5
    # extra positional / keyword arguments are swallowed, as the reference's *_args, **_kwargs do
    assert repr(getattr(A, cls)(3, **{k: v for k, v in DEFAULTS[cls].items() if k in ("box_min", "translate_max")},
                                unused=1)) == aug_cases.REPR[cls]
    seq = A.AugmentationSequence([aug, A.IdentityAug(5)])
    assert repr(seq) == f"AugmentationSequence: ({[aug_cases.REPR[cls], 'Identity']})"
    assert seq.device_chain() is not None and seq.single_shift() is None and not seq.is_identity()


def test_parameter_dtypes_match_the_reference():
    A = _ssa().augmentations
    t = A.TranslateAug(4)
    assert t.translation.dtype == torch.int32 and t.translation.shape == (4, 2)
    assert t.random_color.dtype == torch.float32 and t.random_color.shape == (4, 3, 1, 1)
    cc = A.CutoutColorAug(4)
    assert cc.rand_box.dtype == torch.float32 and cc.rand_box.shape == (4, 3, 1, 1) and cc.w1.dtype == torch.int64
    assert A.GammaAug(4).gamma.shape == (4, 1, 1, 1) and A.GammaAug(4).gamma.dtype == torch.float32
    assert A.HorizontalFlipAug(4).random_inds.dtype == np.bool_
    r = A.RotateAug(4)
    assert torch.is_tensor(r.random_inds) and r.random_inds.dtype == torch.int64


@pytest.mark.parametrize("name", sorted(aug_cases.CASES))
def test_seeded_draws_follow_the_reference(name):
    """construction + one change_randomization_params() of the sequence: the recorded parameters, and the torch, numpy and
    Python generators left where the reference left them (the probes drawn right after its call)"""
    A = _ssa().augmentations
    spec, rec = aug_cases.CASES[name], aug_cases.load(name)
    seed = int(rec["seed"])
    torch.manual_seed(seed); np.random.seed(seed); random.seed(seed)
    augs = aug_cases.build(A, spec)
    A.AugmentationSequence(augs).change_randomization_params()
    for key, have in aug_cases.snapshot(augs, spec).items():
        assert have.dtype == rec[key].dtype and np.array_equal(have, rec[key]), key
    assert np.array_equal(torch.randint(1 << 30, (4,)).numpy(), rec["probe_torch"])
    assert np.array_equal(np.random.randint(1 << 30, size=4), rec["probe_numpy"])
    assert random.random() == float(rec["probe_python"])


def test_rotate_turn_rule_is_the_reference_quirk():
    """random_inds = draw * B + i is compared with k = 1, 2, 3 and turned k + 1 quarter turns: 1 -> 2, 2 -> 3, 3 -> none"""
    A = _ssa().augmentations
    r = A.RotateAug(6)
    r.random_inds = torch.tensor([0, 1, 2, 3, 10, 23])
    assert r.turns().tolist() == [0, 2, 3, 0, 0, 0]
    r.random_inds = torch.tensor([6, 7, 8, 9, 4, 5])    # a non-zero draw: the value leaves {1, 2, 3}
    assert r.turns().tolist() == [0] * 6
    rec = aug_cases.load("aug_RotateAug_c9")
    r.random_inds = torch.from_numpy(rec["p0_random_inds"])
    assert set(r.turns().tolist()) == {0, 2, 3}


@pytest.mark.parametrize("name", sorted(n for n, s in aug_cases.CASES.items()
                                        if not any(c == "Drqv2Aug" for c, _ in s["members"])))
def test_host_table_reproduces_the_reference(name):
    """the op table the kernel is handed, walked by a numpy restatement of the kernel (aug_cases.walk_table): exact for the
    integer-valued cases; Gamma within rtol 1e-6 (numpy's fp64 power rounded once, as the kernel takes it)"""
    A = _ssa().augmentations
    spec, rec = aug_cases.CASES[name], aug_cases.load(name)
    with aug_cases.DrawReplay(_ssa().rng, spec, rec, repeat=2):
        augs = aug_cases.build(A, spec)
        seq = A.AugmentationSequence(augs)
        seq.change_randomization_params()
    plan = seq.device_chain()
    assert plan is not None and len(plan.members) == len(spec["members"])
    tab = plan.host_table()
    assert tab.dtype == np.int32 and tab.shape == (spec["B"], len(spec["members"]), 8)
    for k in range(2 if spec["both"] else 1):
        got, want = aug_cases.walk_table(tab, rec[f"in{k}"]), rec[f"out{k}"].astype(np.float32)
        if aug_cases.is_exact(spec):
            assert np.array_equal(got, want)
        else:
            edge = (want == 0) | (want == 255)
            assert np.array_equal(got[edge], want[edge])
            assert np.allclose(got[~edge], want[~edge], rtol=1e-6, atol=0)


def test_fixtures_show_what_they_are_there_for():
    rec = aug_cases.load("aug_GammaAug_c9")
    g = rec["p0_gamma"].reshape(-1)
    assert (g < 0).any() and (rec["in0"][g < 0] == 0).any() and (rec["out0"][g < 0] == 255).any()
    for nm in ("aug_HorizontalFlipAug_c9", "aug_VerticalFlipAug_c3"):
        sel = aug_cases.load(nm)["p0_random_inds"]
        assert sel.any() and not sel.all()
    rec = aug_cases.load("aug_CutoutAug_c9")
    assert ((4 + 2 * rec["p0_h1"] > 32) | (6 + 2 * rec["p0_w1"] > 32)).any()
    for nm in aug_cases.CASES:
        r = aug_cases.load(nm)
        assert r["in0"].dtype == np.uint8
        assert r["out0"].dtype == (np.uint8 if aug_cases.is_exact(aug_cases.CASES[nm]) else np.float32)


def test_one_table_upload_per_randomisation():
    A = _ssa().augmentations
    seq = A.AugmentationSequence([A.TranslateAug(4), A.IdentityAug(4), A.CutoutColorAug(4), A.GammaAug(4)])
    plan = seq.device_chain()
    assert seq.device_chain() is plan and [type(m).__name__ for m in plan.members] == ["TranslateAug", "CutoutColorAug", "GammaAug"]
    dev = torch.device("cpu")
    t0 = plan.table(dev)
    assert plan.table(dev) is t0                       # cached: no second copy for s'
    seq.change_randomization_params()
    t1 = plan.table(dev)
    assert t1 is not t0 and plan.table(dev) is t1      # one new table per randomisation, whatever the member count
    assert t1.shape == (4, 3, 8) and t1.dtype == torch.int32


def test_mixed_sequence_splits_into_passes():
    A = _ssa().augmentations
    seq = A.AugmentationSequence([A.CutoutAug(4), A.WindowAug(4), A.Drqv2Aug(4), A.HorizontalFlipAug(4)])
    assert seq.device_chain() is None and seq.single_shift() is None
    kinds = [type(p).__name__ for p in seq.device_passes().passes]
    assert kinds == ["_ChainPlan", "Drqv2Aug", "_ChainPlan"]
    assert A.AugmentationSequence([A.Drqv2Aug(4)]).device_passes() is None      # the DrQ path stays what it was
    assert A.AugmentationSequence([A.IdentityAug(4)]).device_passes() is None
    with pytest.raises(AssertionError):
        A._ChainPlan([A.GammaAug(4)] * 9)
    # a DrQ member that adds noise is refused inside a mixed sequence, with its reason
    with pytest.raises(NotImplementedError, match="no HIP path"):
        A.AugmentationSequence([A.DrqAug(4), A.CutoutAug(4)]).device_passes()
    assert A.AugmentationSequence([A.DrqNoNoiseAug(4), A.CutoutAug(4)]).device_passes() is not None


def test_assigning_a_parameter_invalidates_the_uploaded_table():
    A = _ssa().augmentations
    aug = A.CutoutAug(4)
    plan = A._ChainPlan([aug])
    dev = torch.device("cpu")
    t0 = plan.table(dev)
    aug.w1 = torch.tensor([7, 8, 9, 10])            # as a user of the reference's objects may do
    t1 = plan.table(dev)
    assert t1 is not t0 and t1[:, 0, 3].tolist() == [31, 32, 33, 34] and plan.table(dev) is t1


def test_translate_needs_rgb_groups_and_rotate_square_images():
    A = _ssa().augmentations
    with pytest.raises(RuntimeError):
        A.TranslateAug(2)._check_shape(4, 8, 8)
    r = A.RotateAug(4)
    r.random_inds = torch.tensor([0, 1, 2, 3])
    with pytest.raises(RuntimeError):
        r._check_shape(3, 8, 6)     # row 2 turns by 270 degrees
    r.random_inds = torch.tensor([0, 1, 6, 3])
    r._check_shape(3, 8, 6)         # half turns only


# ------------------------------------------------------------------------------------------ adoption
def _stand_in(cls_name, B, state, bases=()):
    """an object that carries the reference class's NAME and attributes, nothing of this package"""
    klass = type(cls_name, bases, {})
    obj = klass()
    obj.batch_size = B
    for k, v in state.items():
        setattr(obj, k, v)
    return obj


def _ref_shaped(B=4):
    return [
        _stand_in("TranslateAug", B, dict(translate_max=4, translation=torch.tensor([[1, -2], [0, 3], [-4, 0], [2, 2]], dtype=torch.int32),
                                           random_color=torch.arange(12.0).reshape(B, 3, 1, 1))),
        _stand_in("CutoutAug", B, dict(box_min=7, box_max=22, pivot_h=12, pivot_w=24, w1=torch.tensor([7, 8, 9, 10]),
                                        h1=torch.tensor([21, 20, 19, 18]))),
        _stand_in("HorizontalFlipAug", B, dict(p_flip=0.5, dim=3, random_inds=np.array([True, False, True, False])),
                  bases=(type("_FlipAug", (), {}),)),
        _stand_in("GammaAug", B, dict(gamma=torch.tensor([1.0, 0.5, -0.2, 2.0]).view(-1, 1, 1, 1))),
        _stand_in("IdentityAug", B, {}),
    ]


class _ForeignSequence:
    def __init__(self, aug_list):
        self.aug_list, self.keys = aug_list, None


def test_adoption_of_reference_shaped_chain_augmentations():
    """raises NotImplementedError on the parent commit: only the DrQ family was adopted there"""
    ssa = _ssa()
    A = ssa.augmentations
    members = _ref_shaped()
    seq = _ForeignSequence(members)
    gen = (torch.get_rng_state(), np.random.get_state()[1].copy(), random.getstate())
    assert ssa.adopt_augmenter(seq) is seq
    assert torch.equal(torch.get_rng_state(), gen[0]) and np.array_equal(np.random.get_state()[1], gen[1])
    assert random.getstate() == gen[2]                                   # no draw consumed
    assert type(seq) is A.AugmentationSequence
    assert [type(m) for m in members] == [A.TranslateAug, A.CutoutAug, A.HorizontalFlipAug, A.GammaAug, A.IdentityAug]
    tab = seq.device_chain().host_table()                                # the state it held is the state that is used
    assert tab[:, 0, 0].tolist() == [A.AUG_TRANSLATE] * 4 and tab[:, 0, 1:3].tolist() == [[1, -2], [0, 3], [-4, 0], [2, 2]]
    assert np.array_equal(tab.view(np.float32)[:, 0, 5:8], np.arange(12.0, dtype=np.float32).reshape(4, 3))
    assert tab[:, 1, 1:5].tolist() == [[33, 54, 31, 38], [32, 52, 32, 40], [31, 50, 33, 42], [30, 48, 34, 44]]
    assert tab[:, 2, 0].tolist() == [A.AUG_HFLIP, A.AUG_NOP, A.AUG_HFLIP, A.AUG_NOP]
    assert np.array_equal(tab.view(np.float32)[:, 3, 5], np.array([1.0, 0.5, -0.2, 2.0], np.float32))
    assert ssa.adopt_augmenter(seq) is seq and type(members[0]) is A.TranslateAug    # idempotent
    # the next randomisation is drawn by this package's class, on the same generators
    torch.manual_seed(3)
    members[0].change_randomization_params()
    torch.manual_seed(3)
    again = A.TranslateAug(4)
    assert torch.equal(members[0].translation, again.translation) and torch.equal(members[0].random_color, again.random_color)


def test_large_translate_is_adopted_as_itself():
    ssa = _ssa()
    base = type("TranslateAug", (), {})
    obj = _stand_in("LargeTranslateAug", 2, dict(translate_max=8, translation=torch.zeros(2, 2, dtype=torch.int32),
                                                 random_color=torch.zeros(2, 3, 1, 1)), bases=(base,))
    ssa.adopt_augmenter(_ForeignSequence([obj]))
    assert type(obj) is ssa.augmentations.LargeTranslateAug and repr(obj) == "LargeTranslate"


def test_a_name_alone_is_not_the_reference_class():
    ssa = _ssa()
    bare = _stand_in("TranslateAug", 4, {})
    with pytest.raises(NotImplementedError, match="no HIP path.*does not carry its state"):
        ssa.adopt_augmenter(_ForeignSequence([bare]))
    assert type(bare).__module__ != ssa.augmentations.__name__           # nothing was swapped


@pytest.mark.parametrize("cls,why", [("GrayscaleAug", "broadcasting"), ("RadAug", "cv2.resize"),
                                     ("ColorJitterAug", "draws inside forward"),
                                     ("NetworkRandomizationAug", "convolution")])
def test_refusals_name_their_reason(cls, why):
    ssa = _ssa()
    with pytest.raises(NotImplementedError, match="no HIP path") as e:
        ssa.adopt_augmenter(_ForeignSequence([_stand_in(cls, 4, {})]))
    assert cls in str(e.value) and why in str(e.value)


def test_install_rebinds_the_chain_augmentations():
    ssa = _ssa()
    fake = types.SimpleNamespace(learning=types.SimpleNamespace(), learning_utils=types.SimpleNamespace(),
                                 replay=types.SimpleNamespace(), augmentations=types.SimpleNamespace())
    ssa.install(fake)
    for cls in aug_cases.CHAIN_CLASSES:
        assert getattr(fake.augmentations, cls) is getattr(ssa.augmentations, cls)
        assert cls in ssa.adopt._AUG_NAMES
    for cls in ("GrayscaleAug", "RadAug", "ColorJitterAug", "NetworkRandomizationAug"):
        assert not hasattr(fake.augmentations, cls)
