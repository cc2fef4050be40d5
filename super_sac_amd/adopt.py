"""Adoption of a FOREIGN agent: an object built by the reference's own ``super_sac.Agent`` (agent.py:43-130) -- or
anything with the same attributes -- handed to this engine's update functions after ``super_sac_amd.install``.

The engine needs a handful of things the reference's classes do not carry; ``adopt_agent`` adds them in place, once:

  critics[i]        ``arena(dev)``: the packed-ensemble view of ``critics[i].nets`` (engine.MlpArena.adopt re-points
                    every ``nn.Parameter.data`` of fc1 / fc2 / out at it; the modules stay the source of truth)
  actors[i]         ``action_size`` (read off the head layer: fc3 -> out/2, out / act_p -> out)
  popart[i]         the reference layer keeps mu / nu / w / b as plain tensors (popart.py:8-20); it is replaced by
                    the device-resident ``popart.PopArtLayer`` initialised from those values
  encoder           ``ssac_identity_key`` when the encoder returns one of its inputs untouched (the scripts' identity
                    encoders, experiments/gym/train_gym.py:18-28), found by probing with the first batch;
                    ``ssac_concat_keys`` when it lays several vector inputs side by side (probe_concat)
  adv_estimator     replaced by ``adv_estimator.AdvantageEstimator`` (same call signature, adv_estimator.py:82-90)
  act_space_size    read off the actor head

Nothing is copied: weights stay in the torch modules' (re-pointed) parameters, so ``agent.save / load``,
``copy.deepcopy(agent)`` and acting through the modules keep working.

The other two objects the training scripts build with the reference's classes are adopted the same way, in place:

  augmenter         a reference ``AugmentationSequence`` (augmentations.py:20-41) whose ``aug_list`` holds DrQ-family,
                    cutout / translate / flip / rotate / window / gamma, colour-jitter / network-randomisation or identity
                    augmentations (matched by class NAME along the MRO, and by the state that class keeps; a colour-jitter
                    object also by the settings the reference itself can run): every element and the sequence itself change
                    class to this package's; batch size, parameters and the CURRENT randomisation (``shift`` / ``w1, h1``
                    / ``translation`` ...) are kept, no host draw is consumed
  buffer            a reference ``ReplayBuffer`` (replay.py:140-190: numpy ``ReplayBufferStorage`` + float64 segment
                    trees): the filled rows move into an HBM-resident storage, the trees' arrays become the
                    ``PrioritySampler``'s, counters carry over, and the object becomes a ``replay.ReplayBuffer`` --
                    later ``buffer.push(...)`` calls of the collection loop land on the device ring
"""
import types

import numpy as np
import torch

from . import engine


def _head(module):
    return engine.MlpArena.linear_triples(module)[2]


def action_size(actor):
    a = getattr(actor, "action_size", None)
    if a is not None:
        return a
    out = _head(actor).out_features
    return out // 2 if hasattr(actor, "fc3") else out  # tanh-normal heads emit (mu, raw log std)


def _critic_arena(self, dev):
    return engine.bind_arena(self, "nets", list(self.nets), dev)


def adopt_agent(agent, device=None):
    """idempotent; returns the agent"""
    if agent.__dict__.get("_ssac_adopted"):
        return agent
    from . import popart as popart_mod
    from .adv_estimator import AdvantageEstimator
    if device is None:
        device = next(agent.actors[0].parameters()).device
    for actor in agent.actors:
        if not hasattr(actor, "action_size"):
            actor.action_size = action_size(actor)
    for critic in agent.critics:
        assert hasattr(critic, "nets"), "critics[i] must hold its Q-networks in `.nets` (agent.py:16-19)"
        if not hasattr(critic, "arena"):
            critic.arena = types.MethodType(_critic_arena, critic)
        if not hasattr(critic, "num_critics"):
            critic.num_critics = len(critic.nets)
    for i, p in enumerate(agent.popart):
        if p and not hasattr(p, "ptr"):
            mine = popart_mod.PopArtLayer(beta=float(p.beta), min_steps=int(p.min_steps), init_nu=float(p.nu))
            st = mine._read()
            st.mu, st.nu, st.w, st.b = float(p.mu), float(p.nu), float(p.w), float(p.b)
            st.t, st.stable = int(p._t), int(bool(p._stable))
            mine._write(st)
            agent.popart[i] = mine.to(device)
    if not hasattr(agent, "act_space_size"):
        agent.act_space_size = action_size(agent.actors[0])
    if not hasattr(agent.adv_estimator, "evaluate"):
        agent.adv_estimator = AdvantageEstimator(
            agent, discrete=bool(agent.discrete),
            discrete_method=getattr(agent.adv_estimator, "discrete_method", "indirect"),
            continuous_method=getattr(agent.adv_estimator, "cont_method", "mean"))
    agent.__dict__["_ssac_adopted"] = True
    return agent


def probe_identity(encoder, obs_dict):
    """identity encoders hand one of their inputs back untouched; remember which (cached on the encoder)"""
    if "ssac_identity_key" in encoder.__dict__ or getattr(encoder, "ssac_identity_key", None) is not None:
        return getattr(encoder, "ssac_identity_key")
    if encoder.__dict__.get("_ssac_probed"):
        return None
    encoder.__dict__["_ssac_probed"] = True
    from . import conv_encoder
    if conv_encoder.find_conv_module(encoder) is not None:
        return None  # a pixel encoder: runs on the HIP convolution engine
    with torch.no_grad():
        out = encoder(obs_dict)
    for key, val in obs_dict.items():
        if isinstance(out, torch.Tensor) and out.data_ptr() == val.data_ptr() and out.shape == val.shape:
            encoder.__dict__["ssac_identity_key"] = key
            return key
    return None


_CONCAT_PROBE_ROWS = 4
MAX_CONCAT_KEYS = 8   # SSAC_MAX_OBS_KEYS of include/ssac_hip.h


def probe_concat(encoder, obs_dict):
    """concatenating encoders lay their vector inputs side by side (``torch.cat([o["goal"], o["obs"]], 1)``): remember the
    order and the widths as ``ssac_concat_keys`` = ((key, width), ...) (cached on the encoder), or None.  Such an encoder
    has no parameter besides the base class's ``have_at_least_one_param`` and no buffer (a running normaliser must not
    take in probe rows); `obs_dict` ({key: tensor with a leading batch axis}: only shapes and the device are read) has at
    least TWO keys (one key handed back is probe_identity's case; one key handed back as a copy keeps the refusal), every
    one a vector; and on four random rows -- from a LOCAL generator, no global random stream moves -- its output is, bit
    for bit, the keys' columns in some order that uses every key exactly once.
    Limitation: the rows are N(0, 1) draws, so arithmetic that is the identity on small finite values -- a clamp at +-10,
    ``nan_to_num`` -- is not seen, and such an encoder would be taken for a pure concatenation."""
    cached = getattr(encoder, "ssac_concat_keys", None)
    if cached is not None:
        return cached
    if encoder.__dict__.get("_ssac_concat_probed") or obs_dict is None:
        return None
    encoder.__dict__["_ssac_concat_probed"] = True
    if not isinstance(encoder, torch.nn.Module) or not callable(encoder):
        return None
    if any(not n.startswith("have_at_least_one_param.") for n, _ in encoder.named_parameters()):
        return None
    if any(True for _ in encoder.buffers()):
        return None
    if not 2 <= len(obs_dict) <= MAX_CONCAT_KEYS or any(v.dim() != 2 or v.shape[1] < 1 for v in obs_dict.values()):
        return None
    widths = {k: int(v.shape[1]) for k, v in obs_dict.items()}
    dev = next(iter(obs_dict.values())).device
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0xC0CA7)
    probe = {k: torch.randn((_CONCAT_PROBE_ROWS, w), generator=gen, dtype=torch.float32).to(dev) for k, w in widths.items()}
    was_training = encoder.training
    try:
        with torch.no_grad():
            out = encoder(dict(probe))
    except Exception:   # noqa: BLE001  (an encoder of another kind may reject vector rows: not a concatenation)
        return None
    finally:
        encoder.train(was_training)
    if not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (_CONCAT_PROBE_ROWS, sum(widths.values())):
        return None
    order, off, left = [], 0, dict(widths)
    while left:
        hit = next((k for k, w in left.items() if torch.equal(out[:, off:off + w], probe[k])), None)
        if hit is None:
            return None
        order.append((hit, left.pop(hit)))
        off += order[-1][1]
    encoder.__dict__["ssac_concat_keys"] = tuple(order)
    return encoder.__dict__["ssac_concat_keys"]


# ------------------------------------------------------------------------------------------ augmenters
_AUG_NAMES = ("Drqv2Aug", "DrqNoNoiseAug", "LargeDrqNoNoiseAug", "LargeDrqAug", "DrqAug", "IdentityAug",
              "CutoutAug", "CutoutColorAug", "LargeTranslateAug", "TranslateAug", "HorizontalFlipAug", "VerticalFlipAug",
              "RotateAug", "WindowAug", "GammaAug", "ColorJitterAug", "NetworkRandomizationAug")

# the reference's augmentations this engine refuses, and why
_AUG_REFUSED = {
    "GrayscaleAug": "the reference's own implementation (augmentations.py:44-80) raises a broadcasting error unless exactly "
                    "1 or 3 rows are selected and is not a per-image grayscale when it does run: there is nothing to be on "
                    "parity with",
    "RadAug": "it resizes with cv2.resize (augmentations.py:129-162), and no reference output exists to match without it",
}


# what an object that has only the NAME of one of these two lacks (the general wording serves every other class)
_AUG_STATE_NOTE = {
    "ColorJitterAug": "it is named like the reference's ColorJitterAug, which keeps four per-row factor vectors and draws "
                      "inside forward() (row selection and transform order, per application: augmentations.py:627, 681), "
                      "but does not carry its state",
    "NetworkRandomizationAug": "it is named like the reference's NetworkRandomizationAug but does not carry the convolution "
                               "the reference's change_randomization_params() leaves",
}


def _own_aug_class(obj):
    from . import augmentations as A
    for klass in type(obj).__mro__:
        if klass.__name__ in _AUG_NAMES:
            return getattr(A, klass.__name__)
    return None


def _refusal(aug):
    for klass in type(aug).__mro__:
        if klass.__name__ in _AUG_REFUSED:
            return f"augmentation {klass.__name__!r} has no HIP path: {_AUG_REFUSED[klass.__name__]}"
    return (f"augmentation {type(aug).__name__!r} has no HIP path; the update engine runs "
            f"{', '.join(_AUG_NAMES)} of super_sac/augmentations.py")


def adopt_augmenter(augmenter):
    """idempotent; returns the augmenter (class-swapped in place when it was built by the reference's classes)"""
    from . import augmentations as A
    if isinstance(augmenter, A.AugmentationSequence):
        return augmenter
    aug_list = getattr(augmenter, "aug_list", None)
    if aug_list is None:
        raise TypeError(f"{type(augmenter).__name__}: expected an AugmentationSequence (augmentations.py:20-41)")
    swaps = []
    for aug in aug_list:
        if isinstance(aug, (A._ShiftAug, A._ChainAug, A._ColourAug, A.IdentityAug)):
            swaps.append(None)
            continue
        mine = _own_aug_class(aug)
        if mine is None:
            raise NotImplementedError(_refusal(aug))
        # the NAME alone does not make it the reference's class: it has to carry that class's state
        need = (("batch_size",) if getattr(mine, "NEEDS_BATCH_SIZE", True) else ()) + tuple(getattr(mine, "REF_STATE", ()))
        missing = [n for n in need if not hasattr(aug, n)]
        if missing:
            note = _AUG_STATE_NOTE.get(mine.__name__, f"it is named like the reference's {mine.__name__} but does not carry "
                                                      "its state")
            raise NotImplementedError(f"augmentation {type(aug).__name__!r} has no HIP path: {note} (missing {missing})")
        if mine is A.ColorJitterAug and A.jitter_refusal(aug):
            raise NotImplementedError(f"augmentation {type(aug).__name__!r} has no HIP path for {A.jitter_refusal(aug)}")
        swaps.append(mine)
    for aug, mine in zip(aug_list, swaps):
        if mine is None:
            continue
        aug.__class__ = mine
        if issubclass(mine, A._ShiftAug):
            aug.__dict__.pop("pad_func", None)   # (nn.ReflectionPad2d of the reference's DrqAug: the kernel pads itself)
            aug._shift_dev = None
            if not hasattr(aug, "noise"):
                aug.noise = False
        aug._adopt_state()
    augmenter.__class__ = A.AugmentationSequence
    return augmenter


# ------------------------------------------------------------------------------------------ replay buffers
def adopt_buffer(buffer, device=None):
    """idempotent; returns the buffer.  A reference-built (numpy) ReplayBuffer becomes a device-resident one in place."""
    from . import replay as R
    from . import device as default_device
    if isinstance(buffer, R.ReplayBuffer):
        return buffer
    need = ("_maxsize", "_storage", "alpha", "beta", "_it_sum", "_it_min", "_max_priority")
    missing = [n for n in need if not hasattr(buffer, n)]
    if missing:
        raise TypeError(
            f"{type(buffer).__name__} is neither a super_sac_amd.replay.ReplayBuffer nor a reference ReplayBuffer "
            f"(replay.py:140-190; missing {missing}).  Build the buffer after `super_sac_amd.install(super_sac)` -- "
            "it rebinds super_sac.replay.ReplayBuffer -- or pass a super_sac_amd.replay.ReplayBuffer.")
    dev = torch.device(device) if device is not None else torch.device(default_device)
    old = buffer._storage
    per = (R.DevicePrioritySampler(buffer._maxsize, buffer.alpha, buffer.beta, dev) if dev.type == "cuda"
           else R.PrioritySampler(buffer._maxsize, buffer.alpha, buffer.beta))
    sum_v, min_v = np.asarray(buffer._it_sum._value, np.float64), np.asarray(buffer._it_min._value, np.float64)
    assert sum_v.shape == (2 * per.cap,) == min_v.shape, "segment trees of an unexpected capacity"
    per.load_state(sum_v, min_v, buffer._max_priority)   # (an np.float32 stays one: it decides the power a push takes)
    storage = None
    if old is not None:
        n = int(old._max_filled)
        storage = R.ReplayBufferStorage(int(old.size), {k: v[0] for k, v in old.s_stack.items()}, old.action_stack[0], dev)
        for dst, src in ([(storage.s_stack[k], old.s_stack[k]) for k in old.s_stack]
                         + [(storage.s1_stack[k], old.s1_stack[k]) for k in old.s1_stack]
                         + [(storage.action_stack, old.action_stack), (storage.reward_stack, old.reward_stack),
                            (storage.done_stack, old.done_stack)]):
            if n:
                dst[:n].copy_(torch.from_numpy(np.ascontiguousarray(src[:n])).to(dst.dtype))
        storage._next_idx, storage._max_filled = int(old._next_idx), n
    calls = int(getattr(buffer, "total_sample_calls", 0))
    for name in ("_it_sum", "_it_min", "_max_priority"):
        buffer.__dict__.pop(name, None)
    buffer.__class__ = R.ReplayBuffer
    buffer._storage, buffer._per, buffer.device = storage, per, dev
    buffer._stager = R._IndexStager(dev) if storage is not None else None
    buffer.total_sample_calls = calls
    return buffer
