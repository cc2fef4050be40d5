"""Shared by the conv-stack encoder tests: encoder stand-ins that carry the attribute names of the reference's MinAtar
example (``conv1``, ``conv2``, ``fc``, ``embedding_dim``, ``forward_rolling``, ``reset_rolling``) and nothing of its text, two
stacks that must be refused, the matching encoder ``kind`` for the CPU oracle (oracle/ssac_oracle.py is not edited: the tests
replace ``orc.encode`` through monkeypatch), float64 references of the forward pass and of every gradient, and the
measured-tolerance rule of the kernel tests (mlp_encoder_cases.measured_bound)."""
import importlib.util

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

import mlp_encoder_cases as mc

measured_bound = mc.measured_bound
CONVS = ((16, 3, 1), (16, 2, 1))   # (out channels, kernel, stride) of the MinAtar stack


def out_hw(h, w, convs=CONVS):
    for _, k, s in convs:
        h, w = (h - k) // s + 1, (w - k) // s + 1
    return h, w


class MinAtarLike(nn.Module):
    """raw frames -> conv 3x3 (C -> 16) -> ReLU -> conv 2x2 (16 -> 16) -> ReLU -> flatten -> fc; `div` 255: the x / 255
    variant"""

    def __init__(self, channels, hw=(10, 10), emb=50, div=1.0, convs=CONVS):
        super().__init__()
        self.have_at_least_one_param = nn.Linear(1, 1)
        self.conv1 = nn.Conv2d(channels, convs[0][0], kernel_size=convs[0][1], stride=convs[0][2])
        self.conv2 = nn.Conv2d(convs[0][0], convs[1][0], kernel_size=convs[1][1], stride=convs[1][2])
        h, w = out_hw(*hw, convs)
        self.fc = nn.Linear(convs[1][0] * h * w, emb)
        self._dim, self._div = emb, div

    @property
    def embedding_dim(self):
        return self._dim

    def forward_rolling(self, obs):
        return self.forward(obs)

    def reset_rolling(self):
        pass

    def middle(self, x):
        return F.relu(x)

    def flatten(self, x):
        return x.flatten(1)

    def forward(self, obs_dict):
        x = obs_dict["obs"]
        if self._div != 1.0:
            x = x / self._div
        x = self.middle(self.conv1(x))
        x = F.relu(self.conv2(x))
        return self.fc(self.flatten(x))


class SigmoidStackLike(MinAtarLike):
    """a sigmoid where the plain stack has its first ReLU: no candidate matches"""

    def middle(self, x):
        return torch.sigmoid(x)


class NhwcFlattenLike(MinAtarLike):
    """the fc reads a channels-last flatten: no candidate matches"""

    def flatten(self, x):
        return x.permute(0, 2, 3, 1).flatten(1)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's encoder kind "convstack"
# ---------------------------------------------------------------------------------------------------------------------
PARAM_KEYS = ("w1", "b1", "w2", "b2", "wf", "bf")


def oracle_encoder(seed, channels, hw=(10, 10), emb=50, div=1.0, convs=CONVS, dtype=torch.float32):
    """encoder dict of the oracle's shape with the new kind "convstack" (seeded weights, scaled like orc.make_mlp)"""
    rng = np.random.RandomState(seed)

    def layer(shape):
        fan_in = int(np.prod(shape[1:]))
        w = (rng.standard_normal(shape) / np.sqrt(fan_in)).astype(np.float32)
        b = (rng.standard_normal((shape[0],)) * 0.05).astype(np.float32)
        return torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)
    (c1, k1, _), (c2, k2, _) = convs
    h, w = out_hw(*hw, convs)
    w1, b1 = layer((c1, channels, k1, k1))
    w2, b2 = layer((c2, c1, k2, k2))
    wf, bf = layer((emb, c2 * h * w))
    return {"kind": "convstack", "key": "obs", "div": float(div), "strides": (convs[0][2], convs[1][2]),
            "p": {"w1": w1, "b1": b1, "w2": w2, "b2": b2, "wf": wf, "bf": bf}}


def stack_maps(x, p, div, strides=(1, 1)):
    """(h1, h2) of the plain stack in the dtype of its parameters"""
    x = x.to(p["w1"].dtype)
    if div != 1.0:
        x = x / div
    h1 = F.relu(F.conv2d(x, p["w1"], p["b1"], stride=strides[0]))
    return h1, F.relu(F.conv2d(h1, p["w2"], p["b2"], stride=strides[1]))


def patched_encode(orc):
    """orc.encode with the kind "convstack" added; every other kind goes to the oracle's own function"""
    stock = orc.encode

    def encode(enc, obs_dict):
        if enc["kind"] != "convstack":
            return stock(enc, obs_dict)
        p = enc["p"]
        _, h2 = stack_maps(obs_dict[enc["key"]], p, enc["div"], enc["strides"])
        return F.linear(h2.flatten(1), p["wf"], p["bf"])
    return encode


def load_encoder(module, enc):
    """the oracle encoder's weights into a stand-in (or nets.ConvStackEncoder)"""
    with torch.no_grad():
        for mod, (wk, bk) in ((module.conv1, ("w1", "b1")), (module.conv2, ("w2", "b2")), (module.fc, ("wf", "bf"))):
            mod.weight.copy_(enc["p"][wk]); mod.bias.copy_(enc["p"][bk])
    return module


def encoder_tensors(enc):
    return {"w1": enc.conv1.weight, "b1": enc.conv1.bias, "w2": enc.conv2.weight, "b2": enc.conv2.bias,
            "wf": enc.fc.weight, "bf": enc.fc.bias}


def reference(x, p, div, dtype, d_flat=None, d_emb=None):
    """forward and every gradient by torch autograd on the CPU in `dtype` (float64: the reference; float32: what the bound is
    measured with).  d_flat: dL/d(flatten), the kernels' input -- gradients of the two conv layers; d_emb: dL/d(embedding),
    the engine's input -- gradients of all six tensors."""
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    h1, h2 = stack_maps(x.to(dtype), q, div)
    flat = h2.flatten(1)
    out = {"h1": h1.detach().flatten(1), "flat": flat.detach()}
    if "wf" in q:
        emb = F.linear(flat, q["wf"], q["bf"])
        out["emb"] = emb.detach()
    if d_flat is not None:
        (flat * d_flat.to(dtype)).sum().backward()
    elif d_emb is not None:
        (emb * d_emb.to(dtype)).sum().backward()
    for k, v in q.items():
        if v.grad is not None:
            out["g" + k] = v.grad.detach()
    return out


def grid_case(seed, B, channels, hw=(10, 10), convs=CONVS):
    """inputs on which every fp32 sum of the two conv layers and their gradients is EXACT in any order: 0/1 pixels, weights,
    biases and d(flat) on a 2^-6 grid in [-1/16, 1/16].  The largest sums -- dW over B <= 64 images of up to 64 pixels, terms
    that are multiples of 2^-12 below 1 -- stay under 2^12, i.e. within 24 bits."""
    rng = np.random.RandomState(seed)
    grid = lambda shape: torch.from_numpy(rng.randint(-4, 5, size=shape).astype(np.float32) / 64.0)
    (c1, k1, _), (c2, k2, _) = convs
    h, w = out_hw(*hw, convs)
    x = torch.from_numpy((rng.uniform(size=(B, channels) + tuple(hw)) < 0.3).astype(np.uint8))
    p = {"w1": grid((c1, channels, k1, k1)), "b1": grid((c1,)), "w2": grid((c2, c1, k2, k2)), "b2": grid((c2,))}
    return x, p, grid((B, c2 * h * w))


def gauss_case(seed, B, channels, hw=(10, 10), emb=50, convs=CONVS):
    """uint8 pixels 0..255 under div = 255, Gaussian weights; d(flat) and d(embedding) Gaussian"""
    rng = np.random.RandomState(seed)
    enc = oracle_encoder(seed, channels, hw, emb, 255.0, convs)
    h, w = out_hw(*hw, convs)
    x = torch.from_numpy(rng.randint(0, 256, size=(B, channels) + tuple(hw)).astype(np.uint8))
    d_flat = torch.from_numpy(rng.standard_normal((B, convs[1][0] * h * w)).astype(np.float32))
    d_emb = torch.from_numpy(rng.standard_normal((B, emb)).astype(np.float32))
    return x, enc["p"], d_flat, d_emb


# ---------------------------------------------------------------------------------------------------------------------
# update sequences: mlp_encoder_cases' oracle / engine drivers (run_oracle, EngineRun, compare) on a conv-stack encoder.
# They find the configuration's pieces -- transitions, the oracle's agent, the encoder module -- through their module's
# globals, so a PRIVATE instance of that module is loaded here and those pieces are replaced in it; the module the
# MLP-encoder tests import is untouched.
# ---------------------------------------------------------------------------------------------------------------------
# seed: as in mlp_encoder_cases -- the straggler allowance is a cap, so the seeds are ones for which the oracle ALONE, fp32
# against fp64, stays inside it on every encoder tensor (tools/vet_conv_stack_seeds.py prints the table)
CONFIGS = {
    "minatar": dict(obs=(4, 10, 10), emb=50, act=6, hidden=64, N=2, E=1, B=8, discrete=True, div=1.0, seed=3),
}
STEPS = mc.STEPS


def transitions(cfg):
    """MinAtar-like frames: uint8, 0/1 valued"""
    rng = np.random.RandomState(cfg["seed"] + 100)
    s = (rng.uniform(size=(mc.ROWS,) + cfg["obs"]) < 0.3).astype(np.uint8)
    s1 = (rng.uniform(size=(mc.ROWS,) + cfg["obs"]) < 0.3).astype(np.uint8)
    a = rng.randint(0, cfg["act"], size=(mc.ROWS, 1)).astype(np.float32)
    r = rng.standard_normal((mc.ROWS,)).astype(np.float32)
    d = rng.uniform(size=(mc.ROWS,)) < 0.05
    return {"obs": s}, a, r, {"obs": s1}, d


def make_encoder(cfg, own=False):
    """the encoder module of a configuration: a stand-in in the reference's shape, or (own) ssa.nets.ConvStackEncoder"""
    if own:
        import super_sac_amd as ssa
        return ssa.nets.ConvStackEncoder(cfg["obs"], CONVS, cfg["emb"], input_div=cfg["div"])
    return MinAtarLike(cfg["obs"][0], cfg["obs"][1:], cfg["emb"], cfg["div"])


def _runner():
    spec = importlib.util.spec_from_file_location("_conv_stack_update_runner", mc.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def oracle_agent(orc, cfg, dtype=torch.float32):
        enc = oracle_encoder(cfg["seed"] + 7, cfg["obs"][0], cfg["obs"][1:], cfg["emb"], cfg["div"])
        oa = orc.AgentOracle(state_dim=cfg["emb"], act_dim=cfg["act"], hidden=cfg["hidden"], num_critics=cfg["N"],
                             ensemble_size=cfg["E"], discrete=True, actor_kind="discrete", popart=False, encoder=enc,
                             seed=cfg["seed"])
        if dtype != torch.float32:
            cast = lambda d: {k: v.to(dtype) for k, v in d.items()}
            oa.actors = [cast(a) for a in oa.actors]
            oa.critics = [[cast(c) for c in ens] for ens in oa.critics]
            oa.encoder = dict(oa.encoder, p=cast(oa.encoder["p"]))
        return oa
    mod.transitions, mod.oracle_agent, mod.make_encoder = transitions, oracle_agent, make_encoder
    mod.load_encoder, mod.encoder_tensors = load_encoder, encoder_tensors
    return mod


runner = _runner()
run_oracle, run_engine, EngineRun, compare = runner.run_oracle, runner.run_engine, runner.EngineRun, runner.compare
