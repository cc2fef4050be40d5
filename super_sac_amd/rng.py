"""Host random streams of the update path, kept on the SAME generators the reference uses
so a run that swaps in this engine consumes them identically:

  replay indices, DrQ shifts      torch CPU default generator   (replay.py:122, augmentations.py:227)
  REDQ target subset, logged net  Python ``random``             (agent.py:29, learning.py:135)
  action noise eps                generator of the compute device (distributions: Normal.sample)
  Beta policy draws x             the agent's engine Philox stream, inside ssac_beta_fwd (beta_dist=True)

Beta draws are the one exception to "the same generators": the reference draws them with torch's CPU Gamma sampler
(torch._sample_dirichlet), and reproducing that sampler bit for bit is not a goal.  They come from the agent's engine
stream instead (Marsaglia-Tsang in the kernel, include/ssac_hip.h: ssac_beta_fwd), one counter per draw site in the
agent's checkpointed noise list (beta.SITES), so a saved and resumed run continues the stream.

Parity tests replace these functions to replay the draws recorded in tests/golden.
"""
import random

import torch


def draw_indices(n, batch_size):
    return torch.randint(n, (batch_size,))


def draw_subset(num_critics, k):
    return random.sample(range(num_critics), k=k)


def choice(seq):
    return random.choice(seq)


def draw_normal(shape, device):
    return torch.randn(*shape, device=device)


def draw_normal_into(dst):
    """standard-normal draw written in place (same device-generator consumption as torch.randn)."""
    return dst.normal_()


_stock_draw_normal, _stock_draw_normal_into = draw_normal, draw_normal_into


def normal_is_stock():
    """True while no test hook replaces the device-noise draws: only then may a consumer switch to the engine's
    in-kernel Philox stream ("device noise from an engine Philox stream; parity tests inject eps")."""
    return draw_normal is _stock_draw_normal and draw_normal_into is _stock_draw_normal_into


def draw_beta_into(dst):
    """injection hook of the Beta policy draws: a replacement writes x in (0, 1) -- the Beta sample BEFORE the action
    transform a = 2x - 1 -- into dst (n_rows x act_dim, on the device) in place, one call per draw site, in the
    reference's call order.  The stock function is never called: while it is in place (beta_is_stock()) the kernel
    draws x from the agent's engine stream itself."""
    raise RuntimeError("rng.draw_beta_into is an injection hook: stock Beta draws come from the engine stream in "
                       "ssac_beta_fwd")


_stock_draw_beta_into = draw_beta_into


def beta_is_stock():
    """True while no test hook replaces the Beta draws (then ssac_beta_fwd draws from the agent's Philox stream)."""
    return draw_beta_into is _stock_draw_beta_into


def draw_categorical(logits):
    """Categorical(logits=logits).sample() on the logits' device (learning_utils.py:386-388, softmax backup weights of
    a discrete agent): index plumbing on torch's device generator, as the reference draws it."""
    return torch.distributions.Categorical(logits=logits).sample()


def draw_permutation(n):
    """torch.randperm(n) on the CPU default generator (the negatives of the contrastive Markov loss, learning.py:300)."""
    return torch.randperm(n)


def draw_drqv2_shift(batch_size, pad):
    return torch.randint(0, 2 * pad + 1, size=(batch_size, 1, 1, 2))


def draw_drq_offsets(batch_size, pad):
    w1 = torch.randint(0, pad * 2, (batch_size,))
    h1 = torch.randint(0, pad * 2, (batch_size,))
    return w1, h1
