"""Beta policy head of ``Agent(beta_dist=True)`` (reference nets/distributions.py:18-53, mlps.py:11-42) on the engine.

The actor's fc3 output ``vec`` (n x 2A) is laid out as for the tanh-normal head, so checkpoints interchange;
alpha = 1 + softplus(vec[:, :A]), beta = 1 + softplus(vec[:, A:]), x ~ Beta(alpha, beta), a = 2x - 1.  The arithmetic is
ssac_beta_fwd / ssac_beta_bwd (csrc/ssac_beta.hip); this module is the host side every update / acting path shares:

  sample()      x from the agent's engine stream (or the rng.draw_beta_into hook) -> a, log pi, the saved x
  mean_into()   2 alpha / (alpha + beta) - 1 (Agent.forward)
  given_logp()  log pi of GIVEN actions, x = (clamp(a, +-0.99) + 1) / 2 (behavioural cloning)
  refuse()      the entry points a Beta agent does not take raise NotImplementedError naming Beta

Beta actors always take the per-layer path (engine.mlp_forward + ssac_beta_fwd, engine.mlp_backward + ssac_beta_bwd):
the fused / chained / recorded forms and the acting fast path are tanh-normal kernels and decline them.

Random stream: one key (SITE_SALT) and one counter per draw site (SITES) in the agent's noise list ``_ssac_noise`` (learning_utils.noise_stream:
[seed, critic-update draws, actor-update number, <one counter per site>]), which checkpoint.py saves and restores.
"""
import ctypes as C

import torch

from . import _lib, engine, rng
from ._lib import check, lib

SITES = ("td", "actor", "alpha", "backup", "act")
_BASE = 3   # first site counter's index in _ssac_noise
# each site draws under its own Philox key (the agent's seed ^ the site's salt): draw k of one site and draw k of another
# are independent, as the reference's successive torch._sample_dirichlet calls are
SITE_SALT = tuple((0x9E3779B97F4A7C15 * (j + 1)) & (2 ** 64 - 1) for j in range(len(SITES)))


def is_beta(actor):
    return getattr(actor, "dist_impl", None) == "beta"


def agent_is_beta(agent):
    return not getattr(agent, "discrete", False) and is_beta(agent.actors[0])


def refuse(what):
    raise NotImplementedError(f"{what}: Beta policies (beta_dist=True) are not supported here")


def site_counter(agent, dev, site):
    """(noise list, index of `site`'s counter): the list is padded in place, so a checkpoint of an agent that never drew
    a Beta sample resumes with zero counters and one that did continues where it stopped"""
    from . import learning_utils as lu
    ns = lu.noise_stream(agent, dev)
    while len(ns) < _BASE + len(SITES):
        ns.append(0)
    return ns, _BASE + SITES.index(site)


def sample(agent, vec, n, A, site, x_save, act_dst=None, ld_act=0, col0=0, logp=None):
    """one draw of Beta(alpha, beta) per element of the n x A head output `vec` (n x 2A, row stride 2A): a = 2x - 1 into
    act_dst[:, col0:col0+A] (row stride ld_act), log pi into logp (n,), x into x_save (n x A).  The hook, when a test
    installed one, supplies x (rng.draw_beta_into); otherwise the kernel draws it from the agent's engine stream at this
    site's next draw number."""
    dev = vec.device
    st = engine.stream()
    act_ptr = act_dst.data_ptr() if act_dst is not None else 0
    lp_ptr = logp.data_ptr() if logp is not None else 0
    if rng.beta_is_stock():
        ns, k = site_counter(agent, dev, site)
        rs = _lib.Rng(ns[0] ^ SITE_SALT[k - _BASE], 0, ns[k])
        ns[k] += 1
        check(lib.ssac_beta_fwd(vec.data_ptr(), 2 * A, n, A, 0, 0, 0, C.addressof(rs), act_ptr, ld_act, col0,
                                lp_ptr, x_save.data_ptr(), st))
    else:
        xin = torch.empty(n, A, device=dev)
        rng.draw_beta_into(xin)
        check(lib.ssac_beta_fwd(vec.data_ptr(), 2 * A, n, A, 0, xin.data_ptr(), A, 0, act_ptr, ld_act, col0,
                                lp_ptr, x_save.data_ptr(), st))
    return x_save


def mean_into(vec, n, A, act):
    """act (n x A) = the distribution's mean 2 alpha / (alpha + beta) - 1"""
    check(lib.ssac_beta_fwd(vec.data_ptr(), 2 * A, n, A, 1, 0, 0, 0, act.data_ptr(), A, 0, 0, 0,
                            engine.stream()))
    return act


def given_logp(vec, n, A, act, logp, x_save):
    """log pi (n,) of the given actions act (n x A, any row stride) through the transform's inverse"""
    check(lib.ssac_beta_fwd(vec.data_ptr(), 2 * A, n, A, 2, act.data_ptr(), act.stride(0), 0, 0, 0, 0,
                            logp.data_ptr(), x_save.data_ptr(), engine.stream()))
