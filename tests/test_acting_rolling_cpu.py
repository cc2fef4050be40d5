"""CPU: which encoders the acting path treats as stateless under rolling=True (super_sac_amd/acting.py: _inherits_rolling /
_rolling_passthrough).  An encoder whose rolling interface is the inherited pass-through -- forward_rolling = forward,
reset_rolling a no-op: nets.Encoder here, nets/__init__.py:26-30 of the reference -- computes under rolling=True what it
computes under rolling=False, so the recorded plan serves both; one that overrides either function keeps state and stays on
the general path.  The detection compares function objects and never imports the reference: its Encoder is stood in for
here by a class of the same module and name."""
import torch.nn as nn


def _reference_encoder():
    """a class shaped like the reference's super_sac.nets.Encoder (nets/__init__.py:21-35), module and name included"""
    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.have_at_least_one_param = nn.Linear(1, 1)

        def forward_rolling(self, obs):
            return self.forward(obs)

        def reset_rolling(self):
            pass
    Encoder.__module__ = "super_sac.nets"
    Encoder.__qualname__ = "Encoder"
    return Encoder


def test_the_package_encoders_are_pass_through():
    from super_sac_amd import acting, nets
    assert acting._inherits_rolling(nets.Encoder)
    assert acting._inherits_rolling(nets.PixelEncoder) and acting._inherits_rolling(nets.IdentityEncoder)

    class AtariEncoder(nets.PixelEncoder):   # (a script's subclass that leaves the rolling interface alone)
        def forward(self, obs_dict):
            return super().forward(obs_dict)
    assert acting._inherits_rolling(AtariEncoder)


def test_a_reference_shaped_encoder_is_pass_through_without_importing_the_reference():
    import sys
    from super_sac_amd import acting
    Ref = _reference_encoder()
    before = {m for m in sys.modules if m.split(".")[0] == "super_sac"}

    class DMCPixelEncoder(Ref):              # train_dmc_from_pixels.py:15-27: forward only
        def forward(self, obs_dict):
            return obs_dict["obs"]
    assert acting._inherits_rolling(Ref) and acting._inherits_rolling(DMCPixelEncoder)
    assert {m for m in sys.modules if m.split(".")[0] == "super_sac"} == before

    # the same functions under another module or class name are somebody else's: not recognised
    Other = _reference_encoder()
    Other.__module__ = "somewhere.nets"
    assert not acting._inherits_rolling(type("E", (Other,), {}))
    # and a class without the interface at all
    assert not acting._inherits_rolling(nn.Linear)


def test_an_override_of_either_function_is_stateful():
    from super_sac_amd import acting, nets
    Ref = _reference_encoder()
    for base in (nets.PixelEncoder, nets.Encoder, Ref):
        class Rolls(base):
            def forward_rolling(self, obs):
                return self.forward(obs)     # (the same body is still an override: the function objects differ)

        class Resets(base):
            def reset_rolling(self):
                pass

        class Below(Rolls):                  # (inherits the override)
            pass
        assert not acting._inherits_rolling(Rolls)
        assert not acting._inherits_rolling(Resets)
        assert not acting._inherits_rolling(Below)


def test_the_answer_is_cached_per_encoder_object():
    from super_sac_amd import acting, nets
    enc = nets.IdentityEncoder(3)
    assert "_ssac_roll_pass" not in enc.__dict__
    assert acting._rolling_passthrough(enc) is True and enc.__dict__["_ssac_roll_pass"] is True

    class Stateful(nets.IdentityEncoder):
        def forward_rolling(self, obs):
            return self.forward(obs)
    st = Stateful(3)
    assert acting._rolling_passthrough(st) is False and st.__dict__["_ssac_roll_pass"] is False
    # an override bound on the OBJECT counts as well
    patched = nets.IdentityEncoder(3)
    patched.reset_rolling = lambda: None
    assert acting._rolling_passthrough(patched) is False
