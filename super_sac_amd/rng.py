"""Host random streams of the update path, kept on the SAME generators the reference uses
so a run that swaps in this engine consumes them identically:

  replay indices, DrQ shifts      torch CPU default generator   (replay.py:122, augmentations.py:227)
  cutout / translate / rotate /   torch CPU default generator   (augmentations.py:99, 311, 386, 477, 526)
  window parameters
  flip rows, gamma exponents      numpy's global generator      (augmentations.py:412, 441)
  colour-jitter factors,          torch CPU default generator   (augmentations.py:648-675, 794-798; the reference draws
  network-randomisation conv                                     these on the CUDA generator where CUDA is present)
  colour-jitter rows and order    numpy's global generator, then Python ``random`` (augmentations.py:627, 681), per
                                  application and frame group
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

import numpy as np
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


# ---- chained augmentations (augmentations.py:83-126, 296-534): the reference's generators, in the reference's order
def draw_cutout_box(batch_size, box_min, box_max):
    """CutoutAug (augmentations.py:99-100, 118-119): w1 then h1 on torch's CPU generator"""
    w1 = torch.randint(box_min, box_max, (batch_size,))
    h1 = torch.randint(box_min, box_max, (batch_size,))
    return w1, h1


def draw_cutout_color(batch_size, box_min, box_max):
    """CutoutColorAug (augmentations.py:385-393): w1, h1, then the box colour"""
    w1 = torch.randint(box_min, box_max, (batch_size,))
    h1 = torch.randint(box_min, box_max, (batch_size,))
    rand_box = torch.randint(0, 255, size=(batch_size, 3, 1, 1), dtype=torch.float32)
    return w1, h1, rand_box


def draw_translation(batch_size, translate_max):
    """TranslateAug (augmentations.py:309-316): the (dy, dx) translation, then the border colour"""
    translation = torch.randint(2 * translate_max, (batch_size, 2), dtype=torch.int32) - translate_max
    random_color = torch.randint(255, size=(batch_size, 3, 1, 1)).float()
    return translation, random_color


def draw_flip_rows(batch_size, p):
    """_FlipAug (augmentations.py:440-443): numpy's global generator"""
    return np.random.choice([True, False], batch_size, p=[p, 1 - p])


def draw_rotation(batch_size):
    """RotateAug (augmentations.py:476-480): torch.randint(4) * B + arange(B) -- see augmentations.RotateAug on what the
    reference then does with these values"""
    return torch.randint(4, size=(batch_size,)) * batch_size + torch.from_numpy(np.arange(batch_size))


def draw_window(batch_size, crop_max):
    """WindowAug (augmentations.py:525-527): w1 then h1"""
    w1 = torch.randint(0, crop_max, (batch_size,))
    h1 = torch.randint(0, crop_max, (batch_size,))
    return w1, h1


def draw_gamma(batch_size, mean, std):
    """GammaAug (augmentations.py:411-415): numpy's global generator, cast to float32, shaped (B, 1, 1, 1)"""
    return torch.from_numpy(np.random.normal(mean, std, size=(batch_size,))).float().view(-1, 1, 1, 1)


# ---- colour augmentations (augmentations.py:537-801)
def draw_color_jitter(batch_size, contrast, hue, brightness, saturation):
    """ColorJitterAug.change_randomization_params (augmentations.py:648-675): four ``torch.empty(B).uniform_(lo, hi)``
    vectors in the reference's order -- contrast, hue, brightness, saturation -- on torch's CPU generator.  That is where the
    reference draws them on a machine without CUDA (its ``_device`` is then the CPU); with CUDA it uses the device
    generator.  The fixtures under tests/golden were recorded on the CPU, and a run that swaps in this engine keeps the CPU
    stream on every machine."""
    return tuple(torch.empty(batch_size).uniform_(*r) for r in (contrast, hue, brightness, saturation))


def draw_jitter_order(batch_size, prob):
    """ColorJitterAug.forward + transform (augmentations.py:627, 681-686), ONE application to ONE group of three channels:
    the row selection from numpy's global generator (consumed even at prob == 1), then -- if any row was picked --
    ``random.uniform(0, 1) >= 0.5`` from Python's generator.  True: contrast first, then the HSV block; False: the HSV block
    first.  These are draws per application and per frame group, not per randomisation."""
    picked = np.random.choice([True, False], batch_size, p=[prob, 1 - prob])
    if picked.sum() > 0:
        return random.uniform(0, 1) >= 0.5
    return False


def draw_netrand_conv():
    """NetworkRandomizationAug.change_randomization_params (augmentations.py:794-798): ``Conv2d(3, 3, 3, bias=False,
    padding=1)`` -- its default initialisation consumes torch's CPU generator -- then ``xavier_normal_`` on the weight, as
    the reference does where its ``_device`` is the CPU.  Returns the (3, 3, 3, 3) weight [co][ci][ky][kx]."""
    conv = torch.nn.Conv2d(3, 3, kernel_size=3, bias=False, padding=1)
    torch.nn.init.xavier_normal_(conv.weight.data)
    return conv.weight.data
