"""GPU: the figures of profiles/conv_stack_encoder.md.

  1. the MinAtar encoder (10 x 10 uint8 frames, conv 3x3 (C -> 16), conv 2x2 (16 -> 16), fc 784 -> 50) on
     conv_encoder.ConvEncoderEngine in its two launch forms -- the fused conv-stack launches (STACK_FUSED = "all") against the
     per-layer launches (False) -- forward (with the activations kept) and backward, at B 256 and 32 for C 4 and 10, and
     at the corners of the range the default covers (C 1 and 16, B 1 and 1024);
  2. one eager discrete critic_update per form (C 4, 6 actions, hidden 256, 2 critics, B 32).

Method (that of tools/measure_mlp_encoder.py): device events around windows of REPS back-to-back calls after a warm-up,
ROUNDS windows per form with the forms alternating inside every round; reported per call: median over the rounds and their
min .. max (the spread a difference has to exceed).  Clocks are whatever the device runs at under this load (not pinned);
nothing else is measured in the same process.

    python tools/measure_conv_stack_encoder.py [out.txt]
"""
import copy
import os
import sys
from itertools import chain

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from measure_mlp_encoder import compare, fmt  # noqa: E402  (the windows, the alternation and the report line)

FORMS = (("fused", "all"), ("per-layer", False))
POINTS = [(4, 256), (4, 32), (10, 256), (10, 32), (1, 1), (16, 1), (1, 1024), (16, 1024)]   # (C, B)


def encoder(out):
    import super_sac_amd as ssa
    from super_sac_amd import conv_encoder as ce
    dev = torch.device("cuda", torch.cuda.current_device())
    for C, B in POINTS:
        rng = np.random.RandomState(C + B)
        x = torch.from_numpy((rng.uniform(size=(B, C, 10, 10)) < 0.3).astype(np.uint8)).cuda()
        d_emb = torch.from_numpy(rng.standard_normal((B, 50)).astype(np.float32)).cuda()
        fwd, bwd = {}, {}
        for name, form in FORMS:
            torch.manual_seed(1)
            eng = ce.conv_engine(ssa.nets.ConvStackEncoder((C, 10, 10)).cuda(), dev)
            emb = torch.empty(B, 50, device="cuda")

            def forward(eng=eng, emb=emb, form=form):
                ce.STACK_FUSED = form
                eng.forward(x, emb, 50, save=True)

            def backward(eng=eng):   # (the form is the saved forward's)
                eng.backward(d_emb)
            forward()
            assert eng.saved["fused"] == (form == "all")
            fwd[name], bwd[name] = forward, backward
        out(f"C {C}, B {B}")
        out("   forward (activations kept): " + fmt(compare(fwd)))
        out("   backward (all six gradients): " + fmt(compare(bwd)))


def critic(out):
    import super_sac_amd as ssa
    from super_sac_amd import conv_encoder as ce
    ssa.learning.USE_GRAPHS = False   # (a trainable encoder never reaches the recording)
    C, A, hidden, N, B, rows = 4, 6, 256, 2, 32, 2048
    dev = torch.device("cuda")
    rng = np.random.RandomState(0)
    frames = lambda: {"obs": (rng.uniform(size=(rows, C, 10, 10)) < 0.3).astype(np.uint8)}
    data = (frames(), rng.randint(0, A, (rows, 1)).astype(np.float32), rng.standard_normal(rows).astype(np.float32), frames(),
            rng.uniform(size=rows) < 0.01)
    calls = {}
    for name, form in FORMS:
        buf = ssa.replay.ReplayBuffer(rows, device=dev)
        buf.load_experience(*data)
        ag = ssa.Agent(act_space_size=A, encoder=ssa.nets.ConvStackEncoder((C, 10, 10)),
                       actor_network_cls=ssa.nets.DiscreteActor, critic_network_cls=ssa.nets.DiscreteCritic, discrete=True,
                       ensemble_size=1, num_critics=N, hidden_size=hidden, auto_rescale_targets=False)
        ag.to(dev)
        tg = copy.deepcopy(ag)
        copt = torch.optim.Adam(chain(*(c.parameters() for c in ag.critics)), lr=3e-4)
        eopt = torch.optim.Adam(ag.encoder.parameters(), lr=1e-4)
        la = torch.zeros(1, device=dev, requires_grad=True)
        aug = ssa.augmentations.AugmentationSequence([ssa.augmentations.IdentityAug(B)])

        def call(buf=buf, ag=ag, tg=tg, copt=copt, eopt=eopt, la=la, aug=aug, form=form):
            ce.STACK_FUSED = form
            ssa.learning.critic_update(
                buffer=buf, agent=ag, target_agent=tg, critic_optimizer=copt, encoder_optimizer=eopt, log_alphas=[la],
                batch_size=B, gamma=0.99, critic_clip=10.0, encoder_clip=40.0, target_critic_ensemble_n=N,
                weighted_bellman_temp=None, weight_type=None, pop=False, augmenter=aug, encoder_lambda=0,
                random_process=None, noise_clip=None, aug_mix=0.0, discrete=True)
        calls[name] = call
    out(f"eager discrete critic_update, C {C}, 10 x 10, A {A}, hidden {hidden}, {N} critics, B {B} "
        "(host-bound: wall time per call)")
    out("   " + fmt(compare(calls, reps=50)))


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    path = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if path:
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")
    from measure_mlp_encoder import REPS, ROUNDS, WARM
    out(f"device: {torch.cuda.get_device_name(0)}; REPS {REPS}, ROUNDS {ROUNDS}, warm-up {WARM}")
    encoder(out)
    critic(out)


if __name__ == "__main__":
    main()
