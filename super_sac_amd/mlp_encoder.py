"""Two-layer MLP encoders on the HIP path: the reference's ``SharedEncoder`` (``--shared_encoder`` of
experiments/gym/train_gym.py, dmc/train_dmc.py, d4rl/train_d4rl_gym.py: obs -> Linear(dim, 128) -> ReLU ->
Linear(128, dim) -> ReLU) and ``VisgridEncoder`` (experiments/visgrid/train.py: flatten -> Linear(324, 256) -> ReLU ->
Linear(256, 2) -> tanh), and ``nets.MlpEncoder``.

``find_mlp_encoder`` recognises such a module by its structure (exactly two ``nn.Linear``) and confirms the FUNCTION by
probing it once on a few random rows (the precedent is ``adopt.probe_identity``); ``MlpEncoderEngine`` is an
``encoder_base.EncoderEngine`` like the convolution engine, so the update functions only look the engine up
(``encoder_base.encoder_engine``).

Three forms, switched by ``USE_FUSED`` and ``USE_ROWS`` (the tests' A/B, not user configuration):
    per layer   ssac_linear_fwd twice + ssac_enc_act_fwd; ssac_enc_act_bwd, ssac_linear_dgrad_masked and the split-K
                weight-gradient launches (every shape)
    fused       ssac_enc_mlp2_fwd / ssac_enc_mlp2_bwd: both layers in one launch each, the hidden tile kept in LDS,
                followed by the same weight-gradient launches.  The default only where it measured faster
                (ssac_enc_mlp2_supported: the forward at K <= 32); the fused backward runs under USE_FUSED = "all" only
    rows        ssac_enc_mlp2_fwd_rows: the forward of 1 .. 16 rows that keeps nothing for a backward (an acting call, a
                module's own forward): no MFMA tile, layer 1 spread over H / 4 workgroups, layer 2 by the last of them to
                arrive.  The default only where ssac_enc_mlp2_rows_supported says it measured faster; USE_ROWS = "all"
                runs it wherever it is covered.  Never taken with save=True: the update paths keep their forms
"""
import torch
from torch import nn

from . import engine
from ._lib import check, lib
from .encoder_base import EncoderEngine, arena_layout, cached_engine  # noqa: F401  (arena_layout stays importable here)

# True: ssac_enc_mlp2_fwd where ssac_enc_mlp2_supported says it measured faster than the per-layer launches
# (profiles/mlp_encoder.md); False: every layer on its own launches; "all": both fused launches, forward AND backward,
# wherever the shape is covered -- the fused backward measured faster at no shape, so only this setting runs it
USE_FUSED = True
# True: ssac_enc_mlp2_fwd_rows for save=False forwards where ssac_enc_mlp2_rows_supported says it measured faster than the
# form the call would take otherwise (profiles/mlp_encoder.md, "Acting"); False: never; "all": wherever it is covered
USE_ROWS = True
ROWS_SCRATCH = 4 + 16 * 256   # SSAC_ENC_ROWS_SCRATCH: the arrival counter and the hidden rows of the few-row forward
WGRAD_SLICES = 8         # split-K slices of a weight-gradient product, at most
WGRAD_MIN_ROWS = 64      # rows per slice, at least

ACTS = {"none": 0, "relu": 1, "tanh": 2}
_PROBE_ROWS = 4
_PROBE_TOL = 1e-6
# parameter-free modules that may sit between / behind the two Linears (what they compute is settled by the probe)
_PASSIVE = (nn.ReLU, nn.Tanh, nn.Flatten, nn.Identity, nn.Sequential, nn.ModuleList)


def _apply_act(name, t):
    return torch.relu(t) if name == "relu" else torch.tanh(t) if name == "tanh" else t


def _structure(encoder):
    """(lin0, lin1) when, apart from the base class's dummy Linear(1, 1), the module tree holds exactly two nn.Linear (in
    registration order, chained, the second as wide as the embedding) and nothing else that carries state"""
    if not isinstance(encoder, nn.Module) or not hasattr(encoder, "embedding_dim"):
        return None
    dummy = getattr(encoder, "have_at_least_one_param", None)
    lins = []
    for m in encoder.modules():
        if m is encoder or m is dummy:
            continue
        if isinstance(m, nn.Linear):
            lins.append(m)
        elif not isinstance(m, _PASSIVE):
            return None
    if any(True for _ in encoder.parameters(recurse=False)) or any(True for _ in encoder.buffers(recurse=False)):
        return None
    if len(lins) != 2 or lins[0].bias is None or lins[1].bias is None:
        return None
    lin0, lin1 = lins
    try:
        emb = int(encoder.embedding_dim)
    except Exception:
        return None
    if lin0.out_features != lin1.in_features or lin1.out_features != emb:
        return None
    if lin0.weight.dtype != torch.float32 or lin1.weight.dtype != torch.float32:
        return None
    return lin0, lin1


def find_mlp_encoder(encoder, obs_dict=None):
    """(lin0, lin1, act2, key) of a two-layer MLP encoder, or None.  `obs_dict` ({key: tensor with a leading batch axis})
    tells which observation key feeds it: exactly one must flatten to lin0.in_features per row (without it the module's
    own ``ssac_obs_key`` or the reference scripts' "obs" is tried).  The outcome is cached on the encoder; the probe
    draws from a LOCAL generator and leaves every global random stream untouched."""
    if not isinstance(encoder, nn.Module):
        return None
    cached = encoder.__dict__.get("_ssac_mlp_desc")
    if cached is not None:
        return cached or None
    if getattr(encoder, "ssac_identity_key", None) is not None:
        return None
    from . import conv_encoder
    if conv_encoder.find_conv_module(encoder) is not None:
        return None
    st = _structure(encoder)
    if st is None:
        encoder.__dict__["_ssac_mlp_desc"] = False
        return None
    lin0, lin1 = st
    K = lin0.in_features
    declared = getattr(encoder, "ssac_mlp_act", None)
    if declared is not None:
        # nets.MlpEncoder: a parameter container whose forward IS this engine, with its key -- nothing to probe
        desc = (lin0, lin1, declared, encoder.ssac_obs_key) if declared in ACTS else False
        encoder.__dict__["_ssac_mlp_desc"] = desc
        return desc or None
    if obs_dict is not None:
        shapes = {k: tuple(v.shape[1:]) for k, v in obs_dict.items()}
        cands = [k for k, v in obs_dict.items() if v.dim() >= 2 and v[0].numel() == K]
        if len(cands) != 1:
            encoder.__dict__["_ssac_mlp_desc"] = False
            return None
        key = cands[0]
    else:
        key = getattr(encoder, "ssac_obs_key", "obs")
        shapes = {key: (K,)}
    dev = lin0.weight.device
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0x5eed)
    probe = {k: torch.randn((_PROBE_ROWS,) + s, generator=gen, dtype=torch.float32).to(dev) for k, s in shapes.items()}
    was_training = encoder.training
    try:
        with torch.no_grad():
            out = encoder(probe)
            h = torch.relu(nn.functional.linear(probe[key].flatten(1), lin0.weight, lin0.bias))
            z = nn.functional.linear(h, lin1.weight, lin1.bias)
    except Exception:
        if obs_dict is None:
            return None   # (the guessed key may be wrong: decide when the observations are known)
        encoder.__dict__["_ssac_mlp_desc"] = False
        return None
    finally:
        encoder.train(was_training)
    desc = False
    if torch.is_tensor(out) and out.shape == z.shape:
        for name in ("relu", "tanh", "none"):
            if bool(((out.float() - _apply_act(name, z)).abs() <= _PROBE_TOL).all()):
                desc = (lin0, lin1, name, key)
                break
    if desc:
        encoder.__dict__["ssac_obs_key"] = key
    encoder.__dict__["_ssac_mlp_desc"] = desc
    return desc or None


class MlpEncoderEngine(EncoderEngine):
    moments_key = "mlp_encoder"

    def __init__(self, encoder, desc, device):
        self.module = encoder
        self.lin0, self.lin1, self.act_name, self.key = desc
        self.act2 = ACTS[self.act_name]
        self.K, self.H, self.emb = self.lin0.in_features, self.lin0.out_features, self.lin1.out_features
        # the base class's dummy Linear(1, 1) never receives a gradient (torch's Adam skips it) and stays outside the arena
        self._pack([self.lin0.weight, self.lin0.bias, self.lin1.weight, self.lin1.bias], device)

    def fused(self, M):
        """the forward of an M-row batch takes the fused launch"""
        if USE_FUSED == "all":
            return bool(lib.ssac_enc_mlp2_covered(M, self.K, self.H, self.emb))
        return bool(USE_FUSED and lib.ssac_enc_mlp2_supported(M, self.K, self.H, self.emb))

    def rows(self, M):
        """the forward of an M-row batch that saves nothing takes the few-row launch"""
        if USE_ROWS == "all":
            return bool(lib.ssac_enc_mlp2_rows_covered(M, self.K, self.H, self.emb))
        return bool(USE_ROWS and lib.ssac_enc_mlp2_rows_supported(M, self.K, self.H, self.emb))

    def fused_backward(self, M):
        return USE_FUSED == "all" and bool(lib.ssac_enc_mlp2_covered(M, self.K, self.H, self.emb))

    # ------------------------------------------------------------------------------------
    def forward(self, x, dst, ld_dst, save):
        """x (B, ...) fp32 on the device, K values per row: a row-major matrix with any row stride, or any contiguous
        shape (flattened); writes the embedding into dst[:, :emb] (row stride ld_dst).  With `save`, keeps what backward()
        needs."""
        engine.require_gpu(x)
        if x.dtype != torch.float32:
            raise NotImplementedError(f"MLP encoder on {x.dtype} observations: the HIP path reads float32 rows")
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1]:
            ldx = x.stride(0)
        else:
            x = x.contiguous()
            ldx = self.K
        self.forward_ptr(x.data_ptr(), tuple(x.shape), 0, dst.data_ptr(), ld_dst, save, img=x, dst=dst, ldx=ldx)

    def forward_ptr(self, x_ptr, shape, u8, dst_ptr, ld_dst, save, img=None, dst=None, ldx=None):
        """forward() on a raw device pointer ((B, ...) fp32, `ldx` floats between rows, default K).  Every launch reads /
        writes workspace buffers keyed by shape: recordable."""
        B = int(shape[0])
        per_row = 1
        for s in shape[1:]:
            per_row *= int(s)
        assert per_row == self.K and not u8, "MLP encoder: expected float32 rows of lin0.in_features values"
        ldx = self.K if ldx is None else int(ldx)
        st = engine.stream()
        K, H, N = self.K, self.H, self.emb
        if not save and self.rows(B):
            # (the scratch block is zeroed once, when the workspace makes it; every launch leaves its counter at zero)
            scratch = self.ws.get("t.rows", (ROWS_SCRATCH,), zero=True)
            check(lib.ssac_enc_mlp2_fwd_rows(x_ptr, ldx, self.lin0.weight.data_ptr(), self.lin0.bias.data_ptr(),
                                             self.lin1.weight.data_ptr(), self.lin1.bias.data_ptr(), B, K, H, N, self.act2,
                                             dst_ptr, ld_dst, scratch.data_ptr(), st))
            return
        hs = self.ws.get("s.h" if save else "t.h", (B, H))
        fused = self.fused(B)
        if fused:
            check(lib.ssac_enc_mlp2_fwd(x_ptr, ldx, self.lin0.weight.data_ptr(), self.lin0.bias.data_ptr(),
                                        self.lin1.weight.data_ptr(), self.lin1.bias.data_ptr(), B, K, H, N, self.act2,
                                        hs.data_ptr() if save else 0, dst_ptr, ld_dst, st))
        else:
            check(lib.ssac_linear_fwd(x_ptr, ldx, self.lin0.weight.data_ptr(), K, self.lin0.bias.data_ptr(),
                                      hs.data_ptr(), H, B, H, K, 1, st))
            check(lib.ssac_linear_fwd(hs.data_ptr(), H, self.lin1.weight.data_ptr(), H, self.lin1.bias.data_ptr(),
                                      dst_ptr, ld_dst, B, N, H, 1 if self.act2 == ACTS["relu"] else 0, st))
            if self.act2 == ACTS["tanh"]:
                check(lib.ssac_enc_act_fwd(dst_ptr, ld_dst, B, N, self.act2, st))
        if save:
            self.saved = dict(B=B, x=img, x_ptr=x_ptr, ldx=ldx, h=hs, out=dst, out_ptr=dst_ptr, ld_out=ld_dst, fused=fused,
                              fused_bwd=self.fused_backward(B))

    # ------------------------------------------------------------------------------------
    def _wgrad(self, dz, ld_dz, x_ptr, ldx, n_out, n_in, B, k_w, k_b, st):
        """dW (n_out x n_in) = dz^T x, db = column sums of dz, into the gradient arena: split over the rows, reduced in a
        fixed order"""
        slices = max(1, min(WGRAD_SLICES, B // WGRAD_MIN_ROWS))
        rps = ((B + slices - 1) // slices + 31) // 32 * 32
        slices = (B + rps - 1) // rps
        gw, gb = self._seg(k_w, self.grads), self._seg(k_b, self.grads)
        if slices == 1:
            check(lib.ssac_linear_wgrad_splitk(dz.data_ptr(), ld_dz, x_ptr, ldx, gw.data_ptr(), gb.data_ptr(), n_out, n_in,
                                               B, B, st))
            return
        pw = self.ws.get(f"b.pw{k_w}", (slices * n_out * n_in,))
        pb = self.ws.get(f"b.pb{k_w}", (slices * n_out,))
        check(lib.ssac_linear_wgrad_splitk(dz.data_ptr(), ld_dz, x_ptr, ldx, pw.data_ptr(), pb.data_ptr(), n_out, n_in, B,
                                           rps, st))
        check(lib.ssac_reduce_slices_pair(pw.data_ptr(), n_out * n_in, gw.data_ptr(), pb.data_ptr(), n_out, gb.data_ptr(),
                                          slices, st))

    def _backward(self, d_rep):
        sv = self.saved
        assert sv is not None, "backward() needs a forward(save=True)"
        B, st = sv["B"], engine.stream()
        K, H, N = self.K, self.H, self.emb
        assert d_rep.is_contiguous() and tuple(d_rep.shape) == (B, N)
        dz1 = self.ws.get("b.dz1", (B, N))
        dz0 = self.ws.get("b.dz0", (B, H))
        h = sv["h"]
        if sv["fused_bwd"]:
            check(lib.ssac_enc_mlp2_bwd(d_rep.data_ptr(), N, sv["out_ptr"], sv["ld_out"], h.data_ptr(),
                                        self.lin1.weight.data_ptr(), B, H, N, self.act2, dz1.data_ptr(), dz0.data_ptr(), st))
        else:
            check(lib.ssac_enc_act_bwd(d_rep.data_ptr(), N, sv["out_ptr"], sv["ld_out"], B, N, self.act2, dz1.data_ptr(), st))
            # (the hidden layer's ReLU derivative rides in the GEMM's epilogue)
            check(lib.ssac_linear_dgrad_masked(dz1.data_ptr(), N, self.lin1.weight.data_ptr(), H, h.data_ptr(), H,
                                               dz0.data_ptr(), H, B, H, N, st))
        self._wgrad(dz1, N, h.data_ptr(), H, N, H, B, 2, 3, st)
        self._wgrad(dz0, H, sv["x_ptr"], sv["ldx"], H, K, B, 0, 1, st)


def mlp_engine(encoder, device, obs_dict=None):
    """MlpEncoderEngine of `encoder` (cached on the encoder under encoder_base.cached_engine's rule), or None when it is no
    two-layer MLP encoder"""
    desc = find_mlp_encoder(encoder, obs_dict)
    if desc is None:
        return None
    return cached_engine(encoder, "_ssac_mlp", device, lambda dev: MlpEncoderEngine(encoder, desc, dev))


def is_mlp_encoder(encoder):
    """recognised already (no probe here: an encoder nobody has looked at yet answers False)"""
    return bool(isinstance(encoder, nn.Module) and encoder.__dict__.get("_ssac_mlp_desc"))
