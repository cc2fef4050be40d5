"""Pixel encoders on the HIP path (reference super_sac/nets/cnns.py:37-103).

``BigPixelEncoder`` (DrQ: conv3x3 s2 + 3x conv3x3 s1, ReLU, fc, LayerNorm, tanh; input x/255-0.5) and
``SmallPixelEncoder`` (Nature-DQN: conv8 s4, conv4 s2, conv3 s1, ReLU, fc; input x/255) run as

    im2col (normalisation fused) -> exact-fp32 MFMA GEMM with bias+ReLU epilogue      per conv layer
    im2col with kernel = whole map -> GEMM                                            fc over the NCHW flatten
    LayerNorm+tanh kernel                                                             (Big only)

with channels-last activations, so each GEMM output is the next layer's input and the
``nn.Conv2d`` weights are used in place as (out, c*kh*kw) matrices.  The backward pass mirrors it
(GEMM backward-data -> col2im with the ReLU mask fused; split-K weight-gradient GEMMs reduced in a
fixed order).  The parameter arena, the accumulate form of backward and the clip + Adam tail are
``encoder_base.EncoderEngine``'s.
"""
import copy
import math

import torch
from torch import nn

from . import engine
from ._lib import check, lib
from .encoder_base import EncoderEngine, cached_engine

USE_IMPLICIT = True          # implicit-GEMM inner conv layers (False: every layer as im2col + GEMM; the tests' A/B)
USE_IMPLICIT_FIRST = True    # the first layer as an implicit GEMM over the NCHW image
FC_CHANNELS_LAST = True      # fc reads the last map in place
IMPLICIT_MIN_ROWS = 16_384       # output pixels (B*Ho*Wo) from which the implicit-GEMM kernels pay off
IMPLICIT_ROWS_PER_SLICE = 256    # output pixels per weight-gradient slice (= per workgroup), at least
FIRST_MIN_ROWS = 16_384          # output pixels from which the first layer leaves im2col
FIRST_ROWS_PER_SLICE = 512       # output pixels per first-layer weight-gradient slice, at least
IMPLICIT_WG_PER_CU = 2           # weight-gradient workgroups per CU (248 VGPRs: at most two waves per SIMD) ...
IMPLICIT_WG_BIG_ROWS = 300_000   # ... and ONE from this many output pixels on (measured: DMC 3.31 -> 3.25 ms; fewer,
                                 # longer slices amortise the cross-wave sum and the partial-slice traffic)
FIRST_WG_PER_CU = 2              # (measured 2 / 3 / 4 / 6: Atari 1.57 / 1.59 / 1.61 / 1.61 ms)
FIRST_WGRAD_BANDS = True         # conv1's weight gradient with the image staged through LDS where covered (DMC: 116 -> 86 us)
WGRAD_WHOLE_IMAGES = True        # weight gradients of layers with small feature maps: x and dy of an image staged in LDS
FC_STREAM = True  # the fc forward as an operand stream (N <= 64 outputs; DMC 49 -> 38 us per pass)
FC_SLICES = 48  # K slices of the tiled fc forward (8 row tiles x 48 slices ~ 1.5 workgroups per CU at B 512)
ROWS_PER_SLICE = 4096  # split-K granularity of the convolution weight gradients
# plain two-layer conv stacks (MinAtar): True: ssac_enc_convstack_fwd / _bwd where ssac_enc_convstack_supported says they
# measured faster than the per-layer launches (profiles/conv_stack_encoder.md); False: every layer on its own launches;
# "all": the fused launches wherever the geometry is covered (the tests' switch)
STACK_FUSED = True
STACK_BWD_MIN_ROWS = 32   # batch from which a pass that keeps its activations (a backward follows) takes the fused form: the
                          # fused backward measured faster at B 32 .. 1024 and slower at B 1 (54 against 41 us at C 16)
STACK_TILE = 4   # images per workgroup of the fused launches (SSAC_ENC_CONVSTACK_TILE): one weight-gradient partial each

_KNOWN_PIXEL = ("BigPixelEncoder", "SmallPixelEncoder")   # cnns.py:37-103: their input normalisation is known, not probed
_STACK_INPUTS = ((1.0, 0.0), (255.0, 0.0))                # (div, shift) candidates of a plain conv stack: raw, x / 255
_PROBE_ROWS = 4
_PROBE_TOL = 1e-5


def _stack_layers(m):
    """(convs, fc) when `m` has the STRUCTURE of a plain conv stack: conv1..convN (N <= 4, no gap) of square, unpadded,
    undilated, ungrouped fp32 nn.Conv2d that chain, an nn.Linear fc, no ln; else None"""
    names = [n for n in ("conv1", "conv2", "conv3", "conv4") if hasattr(m, n)]
    if not names or names != ["conv1", "conv2", "conv3", "conv4"][:len(names)] or hasattr(m, "conv5") or hasattr(m, "ln"):
        return None
    convs, fc = [getattr(m, n) for n in names], getattr(m, "fc", None)
    if not isinstance(fc, nn.Linear) or fc.bias is None or fc.weight.dtype != torch.float32:
        return None
    for c in convs:
        if not isinstance(c, nn.Conv2d) or c.bias is None or c.weight.dtype != torch.float32:
            return None
        if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or c.groups != 1:
            return None
        if tuple(c.dilation) != (1, 1) or c.padding not in ((0, 0), "valid", 0):
            return None
    if any(a.out_channels != b.in_channels for a, b in zip(convs, convs[1:])):
        return None
    return convs, fc


def _probe_shape(m, convs, fc):
    """an input (C, H, W) the stack accepts: the module's own ``ssac_obs_shape``, else the one nearest to a square whose
    last map fills fc.in_features (the frame's true shape is not needed: any accepted size shows what the module computes)"""
    shape = getattr(m, "ssac_obs_shape", None)
    if shape is not None and len(shape) == 3:
        return tuple(int(v) for v in shape)
    pixels, rest = divmod(fc.in_features, convs[-1].out_channels)
    if rest or pixels < 1:
        return None
    h = next(s for s in range(math.isqrt(pixels), 0, -1) if pixels % s == 0)
    w = pixels // h
    for c in reversed(convs):
        h, w = (h - 1) * c.stride[0] + c.kernel_size[0], (w - 1) * c.stride[0] + c.kernel_size[0]
    return convs[0].in_channels, h, w


def stack_function(x, convs, fc, div, shift):
    """fc(flatten_NCHW(relu(convN(... relu(conv1(x / div + shift)))))): what a plain conv stack computes"""
    h = x if div == 1.0 and shift == 0.0 else x / div + shift
    for c in convs:
        h = torch.relu(nn.functional.conv2d(h, c.weight, c.bias, stride=c.stride))
    return nn.functional.linear(h.flatten(1), fc.weight, fc.bias)


def _probe_stack(encoder, m):
    """(div, shift) of the plain conv stack `m` inside `encoder`, or False.  The module's OWN forward is evaluated on a few
    random frames and compared with stack_function for every candidate -- on a CPU copy (no torch convolution runs on the
    GPU on this engine's account) and with a local generator (no global random stream moves)."""
    layers = _stack_layers(m)
    if layers is None:
        return False
    shape = _probe_shape(m, *layers)
    if shape is None:
        return False
    name = next(n for n, sub in encoder.named_modules() if sub is m)
    try:
        cpu = copy.deepcopy(encoder).to("cpu")
    except Exception:
        return False
    cpu_m = cpu.get_submodule(name) if name else cpu
    convs, fc = _stack_layers(cpu_m)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0x5eed)
    x = torch.randint(0, 256, (_PROBE_ROWS,) + shape, generator=gen).to(torch.float32)
    key = getattr(encoder, "ssac_obs_key", "obs")
    with torch.no_grad():
        try:
            out = cpu({key: x})
        except Exception:
            try:
                out = cpu_m(x)
            except Exception:
                return False
        if not torch.is_tensor(out) or tuple(out.shape) != (_PROBE_ROWS, fc.out_features):
            return False
        for div, shift in _STACK_INPUTS:
            if bool(((out.float() - stack_function(x, convs, fc, div, shift)).abs() <= _PROBE_TOL).all()):
                encoder.__dict__.setdefault("ssac_obs_key", key)
                return div, shift
    return False


def find_conv_module(encoder):
    """the convolutional module inside an Encoder wrapper: a BigPixelEncoder / SmallPixelEncoder-shaped one
    (train_dmc_from_pixels.py:15-27 ``conv_block``, train_atari.py:9-20 ``cnn``: by class name, or by its ``ln``), or a
    plain conv stack (experiments/minatar/minatar_utils.py:37-63), whose input normalisation is declared
    (nets.ConvStackEncoder) or found by a one-off probe and cached on the module.  A module with ``conv1`` and ``fc`` that
    is neither raises: it has no HIP path."""
    for m in encoder.modules():
        if hasattr(m, "conv1") and hasattr(m, "fc"):
            if hasattr(m, "ln") or any(k.__name__ in _KNOWN_PIXEL for k in type(m).__mro__):
                return m
            if getattr(m, "ssac_conv_input", None) is not None:
                return m
            found = m.__dict__.get("_ssac_conv_input")
            if found is None:
                found = m.__dict__["_ssac_conv_input"] = _probe_stack(encoder, m)
            if not found:
                raise NotImplementedError(f"{type(encoder).__name__}: this encoder has no HIP path")
            return m
    return None


def conv_input(module):
    """(div, shift) of the first layer's input normalisation x / div + shift"""
    if hasattr(module, "ln"):
        return 255.0, -0.5
    found = getattr(module, "ssac_conv_input", None) or module.__dict__.get("_ssac_conv_input")
    return (float(found[0]), float(found[1])) if found else (255.0, 0.0)


class ConvEncoderEngine(EncoderEngine):
    moments_key = "conv_encoder"

    def __init__(self, module, device):
        self.module = module
        convs = [getattr(module, n) for n in ("conv1", "conv2", "conv3", "conv4") if hasattr(module, n)]
        self.convs = convs
        self.big = hasattr(module, "ln")
        self.geom = [(c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0]) for c in convs]
        self.emb = module.fc.out_features
        # inner layers with 32-multiple channel counts run as implicit GEMMs (csrc/ssac_conv_implicit.hip)
        # (small maps -- decided per call from the row count -- stay on im2col; a strided layer's backward-data pass
        # runs per parity class of input pixels, so no MFMA is spent on a structurally zero tap)
        self.implicit_ok = [USE_IMPLICIT and l > 0 and bool(lib.ssac_conv_implicit_supported(ci, co, k))
                            for l, (ci, co, k, s) in enumerate(self.geom)]
        self.implicit = list(self.implicit_ok)
        self.first = False   # the saved forward ran the first layer as an implicit GEMM
        self.div, self.shift = conv_input(module)
        layers = convs + [module.fc] + ([module.ln] if self.big else [])
        self._pack([p for m in layers for p in (m.weight, m.bias)], device)

    def stack_fused(self, B, H, W, save=False):
        """a B-image batch of H x W frames takes the fused launches of a plain two-layer stack (`save`: forward AND the
        backward that follows it, which is tied to the forward's form)"""
        if not STACK_FUSED or self.big or len(self.geom) != 2:
            return False
        (c, co1, k1, s1), (_, co2, k2, s2) = self.geom
        if STACK_FUSED == "all":
            return bool(lib.ssac_enc_convstack_covered(c, H, W, co1, k1, s1, co2, k2, s2))
        if save and B < STACK_BWD_MIN_ROWS:
            return False
        return bool(lib.ssac_enc_convstack_supported(B, c, H, W, co1, k1, s1, co2, k2, s2))

    # ------------------------------------------------------------------------------------
    def forward(self, img, dst, ld_dst, save):
        """img (B, C, H, W) fp32 on the device; writes the embedding into dst[:, :emb] (row stride
        ld_dst).  With `save`, keeps what backward() needs."""
        engine.require_gpu(img)
        img = img.contiguous()
        self.forward_ptr(img.data_ptr(), tuple(img.shape), 1 if img.dtype == torch.uint8 else 0, dst.data_ptr(), ld_dst, save,
                         img=img, dst=dst)

    def forward_ptr(self, img_ptr, shape, u8, dst_ptr, ld_dst, save, img=None, dst=None):
        """forward() on a raw device pointer: (B, C, H, W) fp32 -- or uint8 (u8 = 1: the cast and the input normalisation
        happen in the first layer's patch gather) -- e.g. the observation buffer of an acting plan (acting.py), which is
        not a torch allocation.  Every launch reads / writes workspace buffers keyed by shape: recordable."""
        B, Cc, Hh, Ww = shape
        st = engine.stream()
        tag = "s" if save else "t"
        fused = self.stack_fused(B, Hh, Ww, save)
        cols, ys, shapes, src, Hf, Wf = (self._forward_stack if fused else self._forward_layers)(img_ptr, shape, u8, tag, save)
        co = self.geom[-1][1]
        flat_dim = co * Hf * Wf
        fc = self.module.fc
        if fused:
            colf, wfc = src, fc.weight
        elif FC_CHANNELS_LAST:
            # the last feature map IS the fc input once the weight's columns are put in channels-last order
            # (emb x C x P -> emb x P x C, 7.8 MB for DrQ: cheaper than gathering B x C*P activations both ways)
            colf = src
            wfc = self.ws.get("fc.wcl", (self.emb * flat_dim,))
            check(lib.ssac_permute_cp(fc.weight.data_ptr(), wfc.data_ptr(), self.emb, co, Hf * Wf, 1, st))
        else:
            colf = self.ws.get(f"{tag}.colf", (B * flat_dim,))
            check(lib.ssac_im2col(src.data_ptr(), 0, Hf * Wf * co, 1, Wf * co, co, B, co, Hf, Wf, Hf, 1, 1.0, 0.0,
                                  colf.data_ptr(), st))
            wfc = fc.weight
        if self.big:
            z = self.ws.get(f"{tag}.z", (B, self.emb))
            self._fc_forward(colf, wfc, B, flat_dim, z.data_ptr(), self.emb)
            xhat = self.ws.get(f"{tag}.xhat", (B, self.emb))
            rstd = self.ws.get(f"{tag}.rstd", (B,))
            ln = self.module.ln
            check(lib.ssac_ln_tanh_fwd(z.data_ptr(), self.emb, ln.weight.data_ptr(), ln.bias.data_ptr(), B,
                                       self.emb, dst_ptr, ld_dst, xhat.data_ptr(), rstd.data_ptr(), st))
        else:
            xhat = rstd = None
            self._fc_forward(colf, wfc, B, flat_dim, dst_ptr, ld_dst)
        if save:
            self.saved = dict(B=B, img=img, img_ptr=img_ptr, u8=u8, shape=(Cc, Hh, Ww), fused=fused, cols=cols, ys=ys,
                              shapes=shapes, colf=colf, wfc=wfc, flat_dim=flat_dim, Hf=Hf, Wf=Wf, xhat=xhat, rstd=rstd,
                              out=dst, ld_out=ld_dst)

    def _forward_stack(self, img_ptr, shape, u8, tag, save):
        """both convolutions of a plain two-layer stack in one launch (csrc/ssac_enc_convstack.hip): the first map goes to
        memory only for backward, the second is written in NCHW flatten order -- the fc's input as its weight is stored"""
        B, Cc, Hh, Ww = shape
        (ci, co1, k1, s1), (_, co2, k2, s2) = self.geom
        Hf, Wf = Hh - k1 + 1 - k2 + 1, Ww - k1 + 1 - k2 + 1
        h1 = self.ws.get("s.h1", (B * co1 * (Hh - k1 + 1) * (Ww - k1 + 1),)) if save else None
        src = self.ws.get(f"{tag}.flat", (B * co2 * Hf * Wf,))
        check(lib.ssac_enc_convstack_fwd(img_ptr, u8, self.convs[0].weight.data_ptr(), self.convs[0].bias.data_ptr(),
                                         self.convs[1].weight.data_ptr(), self.convs[1].bias.data_ptr(), B, Cc, Hh, Ww,
                                         co1, k1, s1, co2, k2, s2, self.div, self.shift, h1.data_ptr() if save else 0,
                                         src.data_ptr(), engine.stream()))
        return [], [h1, src], [], src, Hf, Wf

    def _forward_layers(self, img_ptr, shape, u8, tag, save):
        """every convolution on its own launches; returns (column matrices, channels-last maps, layer shapes, last map, H, W)"""
        B, Cc, Hh, Ww = shape
        st = engine.stream()
        src_ptr = img_ptr
        strides = (Cc * Hh * Ww, Hh * Ww, Ww, 1)
        Hi, Wi, div, shift = Hh, Ww, self.div, self.shift
        cols, ys, shapes = [], [], []
        for l, (ci, co, k, s) in enumerate(self.geom):
            Ho, Wo = (Hi - k) // s + 1, (Wi - k) // s + 1
            rows, ckk = B * Ho * Wo, ci * k * k
            y = self.ws.get(f"{tag}.y{l if save else l % 2}", (rows * co,))
            if save:
                self.implicit[l] = self.implicit_ok[l] and rows >= IMPLICIT_MIN_ROWS
            first = (l == 0 and USE_IMPLICIT_FIRST and rows >= FIRST_MIN_ROWS and not u8 and img_ptr % 16 == 0
                     and lib.ssac_conv_first_supported(ci, co, k, s, Hi, Wi, B) > 0)
            if l == 0 and save:
                self.first = first
            if first:
                # the gather AND the input normalisation happen in the operand loads; the image is what backward reads
                col = None
                check(lib.ssac_conv_first_fwd(img_ptr, self.convs[0].weight.data_ptr(),
                                              self.convs[0].bias.data_ptr(), y.data_ptr(), B, ci, Hi, Wi, co, k, s,
                                              div, shift, st))
            elif self.implicit_ok[l] and rows >= IMPLICIT_MIN_ROWS:
                # channels-last input straight from the previous layer: the patch gather happens in the operand
                # loads of the implicit-GEMM kernel, no column matrix
                col = None
                check(lib.ssac_conv_fwd(src_ptr, self.convs[l].weight.data_ptr(),
                                        self.convs[l].bias.data_ptr(), y.data_ptr(), B, Hi, Wi, ci, co, k, s, st))
            else:
                col = self.ws.get(f"{tag}.col{l if save else 0}", (rows * ckk,))
                check(lib.ssac_im2col(src_ptr, u8 if l == 0 else 0, *strides, B, ci, Hi, Wi, k, s, div, shift,
                                      col.data_ptr(), st))
                check(lib.ssac_linear_fwd(col.data_ptr(), ckk, self.convs[l].weight.data_ptr(), ckk,
                                          self.convs[l].bias.data_ptr(), y.data_ptr(), co, rows, co, ckk, 1, st))
            cols.append(col); ys.append(y); shapes.append((ci, co, k, s, Hi, Wi, Ho, Wo))
            src, src_ptr, strides = y, y.data_ptr(), (Ho * Wo * co, 1, Wo * co, co)  # channels-last view of the GEMM output
            Hi, Wi, div, shift = Ho, Wo, 1.0, 0.0
        return cols, ys, shapes, src, Hi, Wi

    def _fc_forward(self, colf, wfc, B, flat_dim, out_ptr, ld_out):
        """(B x flat_dim) . (emb x flat_dim)^T: 8 x 1 output tiles only -> cut K into slices so the launch fills the chip,
        then a fixed-order reduction adds the bias"""
        fc, st = self.module.fc, engine.stream()
        # few outputs (N <= 64): the operand-stream kernel, one wave per (32 rows, K slice), one workgroup per CU
        row_groups = (B + 127) // 128
        skps = ((flat_dim + max(1, 256 // row_groups) - 1) // max(1, 256 // row_groups) + 7) // 8 * 8
        if FC_STREAM and lib.ssac_linear_fwd_stream_supported(B, self.emb, flat_dim, skps, flat_dim, flat_dim) \
                and (flat_dim + skps - 1) // skps >= 4:
            slices = (flat_dim + skps - 1) // skps
            part = self.ws.get("fc.partial", (slices * B * self.emb,))
            check(lib.ssac_linear_fwd_stream(colf.data_ptr(), flat_dim, wfc.data_ptr(), flat_dim, part.data_ptr(), B,
                                             self.emb, flat_dim, skps, st))
            check(lib.ssac_reduce_slices_bias(part.data_ptr(), slices, B, self.emb, fc.bias.data_ptr(), out_ptr,
                                              ld_out, st))
            return
        kps = max(32, ((flat_dim + FC_SLICES - 1) // FC_SLICES + 31) // 32 * 32)
        slices = (flat_dim + kps - 1) // kps
        if slices < 4:
            check(lib.ssac_linear_fwd(colf.data_ptr(), flat_dim, wfc.data_ptr(), flat_dim,
                                      fc.bias.data_ptr(), out_ptr, ld_out, B, self.emb, flat_dim, 0, st))
            return
        part = self.ws.get("fc.partial", (slices * B * self.emb,))
        check(lib.ssac_linear_fwd_splitk(colf.data_ptr(), flat_dim, wfc.data_ptr(), flat_dim,
                                         part.data_ptr(), B, self.emb, flat_dim, kps, st))
        check(lib.ssac_reduce_slices_bias(part.data_ptr(), slices, B, self.emb, fc.bias.data_ptr(), out_ptr,
                                          ld_out, st))

    # ------------------------------------------------------------------------------------
    def _backward(self, d_rep):
        sv = self.saved
        assert sv is not None, "backward() needs a forward(save=True)"
        B, st = sv["B"], engine.stream()
        if self.big:
            k_fcb = 2 * len(self.geom) + 1
            dz = self.ws.get("b.dz", (B, self.emb))
            scratch = self.ws.get("b.lnscratch", (B, self.emb))
            check(lib.ssac_ln_tanh_bwd(d_rep.data_ptr(), self.emb, sv["out"].data_ptr(), sv["ld_out"],
                                       sv["xhat"].data_ptr(), sv["rstd"].data_ptr(),
                                       self.module.ln.weight.data_ptr(), B, self.emb, dz.data_ptr(), self.emb,
                                       scratch.data_ptr(), self._seg(k_fcb + 1, self.grads).data_ptr(),
                                       self._seg(k_fcb + 2, self.grads).data_ptr(), st))
        else:
            dz = d_rep
        if sv["fused"]:
            self._backward_stack(dz, sv)
        else:
            self._backward_layers(self._backward_fc(dz, sv), sv)

    def _backward_stack(self, dz, sv):
        """fc on the NCHW flatten as it is stored: weight gradient straight into the arena, backward-data, then both layers'
        gradients as one partial per image tile, summed in a fixed order into the arena's first four tensors"""
        B, flat_dim, st = sv["B"], sv["flat_dim"], engine.stream()
        k_fcw, k_fcb = 2 * len(self.geom), 2 * len(self.geom) + 1
        (ci, co1, k1, s1), (_, co2, k2, s2) = self.geom
        Cc, Hh, Ww = sv["shape"]
        check(lib.ssac_linear_wgrad_splitk(dz.data_ptr(), self.emb, sv["colf"].data_ptr(), flat_dim,
                                           self._seg(k_fcw, self.grads).data_ptr(),
                                           self._seg(k_fcb, self.grads).data_ptr(), self.emb, flat_dim, B, B, st))
        dflat = self.ws.get("b.dflat", (B * flat_dim,))
        check(lib.ssac_linear_dgrad(dz.data_ptr(), self.emb, self.module.fc.weight.data_ptr(), flat_dim,
                                    dflat.data_ptr(), flat_dim, B, flat_dim, self.emb, st))
        slices, n = (B + STACK_TILE - 1) // STACK_TILE, self.offs[4]
        assert n == co1 * (ci * k1 * k1 + 1) + co2 * (co1 * k2 * k2 + 1)   # (the four tensors lie back to back)
        part = self.ws.get("b.pstack", (slices * n,))
        check(lib.ssac_enc_convstack_bwd(dflat.data_ptr(), sv["img_ptr"], sv["u8"], sv["ys"][0].data_ptr(),
                                         sv["ys"][1].data_ptr(), self.convs[1].weight.data_ptr(), B, Cc, Hh, Ww, co1, k1,
                                         s1, co2, k2, s2, self.div, self.shift, part.data_ptr(), st))
        check(lib.ssac_reduce_slices(part.data_ptr(), slices, n, self.grads.data_ptr(), st))

    def _backward_fc(self, dz, sv):
        """the fc layer's gradients into the arena; returns dL/d(last map), masked by its ReLU, channels-last"""
        B, flat_dim, st = sv["B"], sv["flat_dim"], engine.stream()
        nconv = len(self.geom)
        k_fcw, k_fcb = 2 * nconv, 2 * nconv + 1
        ci, co, k, s, Hi, Wi, Ho, Wo = sv["shapes"][-1]
        dy = self.ws.get(f"b.dy{(nconv - 1) % 2}", (B * Ho * Wo * co,))
        ylast = sv["ys"][-1]
        if FC_CHANNELS_LAST:
            # fc weight gradient in channels-last column order, then back to the parameter's (C, P) order
            gcl = self.ws.get("fc.gcl", (self.emb * flat_dim,))
            check(lib.ssac_linear_wgrad_splitk(dz.data_ptr(), self.emb, sv["colf"].data_ptr(), flat_dim,
                                               gcl.data_ptr(), self._seg(k_fcb, self.grads).data_ptr(), self.emb,
                                               flat_dim, B, B, st))
            check(lib.ssac_permute_cp(gcl.data_ptr(), self._seg(k_fcw, self.grads).data_ptr(), self.emb, co,
                                      Ho * Wo, 0, st))
            # (the last map's ReLU derivative rides in the GEMM's epilogue: dy is written once, masked)
            check(lib.ssac_linear_dgrad_masked(dz.data_ptr(), self.emb, sv["wfc"].data_ptr(), flat_dim,
                                               ylast.data_ptr(), flat_dim, dy.data_ptr(), flat_dim, B, flat_dim,
                                               self.emb, st))
        else:
            # fc: weight gradient (K = B rows, one slice writes straight into the gradient arena)
            check(lib.ssac_linear_wgrad_splitk(dz.data_ptr(), self.emb, sv["colf"].data_ptr(), flat_dim,
                                               self._seg(k_fcw, self.grads).data_ptr(),
                                               self._seg(k_fcb, self.grads).data_ptr(), self.emb, flat_dim, B, B, st))
            dcolf = self.ws.get("b.dcolf", (B * flat_dim,))
            check(lib.ssac_linear_dgrad(dz.data_ptr(), self.emb, self.module.fc.weight.data_ptr(), flat_dim,
                                        dcolf.data_ptr(), flat_dim, B, flat_dim, self.emb, st))
            cl = (Ho * Wo * co, 1, Wo * co, co)
            check(lib.ssac_col2im(dcolf.data_ptr(), dy.data_ptr(), *cl, ylast.data_ptr(), *cl, B, co, Ho, Wo,
                                  sv["Hf"], 1, st))
        return dy

    def _backward_layers(self, dy, sv):
        """down the convolutions: weight gradient (slices reduced in a fixed order), then backward-data, layer by layer"""
        B, st = sv["B"], engine.stream()
        for l in range(len(self.geom) - 1, -1, -1):
            ci, co, k, s, Hi, Wi, Ho, Wo = sv["shapes"][l]
            rows, ckk = B * Ho * Wo, ci * k * k
            first = l == 0 and self.first
            if first or self.implicit[l]:
                # one slice = one workgroup per (ci/32, co/32) block pair: as many slices as are resident at once (a
                # partly filled second round costs a whole one), never below the configured slice size
                blocks = 1 if first else (ci // 32) * (co // 32)
                per_cu = FIRST_WG_PER_CU if first else 1 if rows >= IMPLICIT_WG_BIG_ROWS else IMPLICIT_WG_PER_CU
                resident = max(1, 256 * per_cu // blocks)
                rps = max(FIRST_ROWS_PER_SLICE if first else IMPLICIT_ROWS_PER_SLICE,
                          ((rows + resident - 1) // resident + 127) // 128 * 128)
            else:
                rps = ROWS_PER_SLICE
            slices = (rows + rps - 1) // rps
            band_slices = int(lib.ssac_conv_first_wgrad_band_slices(B, ci, Hi, Wi, co, k, s)) if first and FIRST_WGRAD_BANDS else 0
            if band_slices:   # (the image staged through LDS in bands of output rows: one partial per persistent workgroup)
                slices = band_slices
            img_slices = (int(lib.ssac_conv_wgrad_img_slices(B, Hi, Wi, ci, co, k, s))
                          if (not first and self.implicit[l] and WGRAD_WHOLE_IMAGES) else 0)
            if img_slices:    # (small feature maps: both operands of an image staged in LDS, one partial per workgroup)
                slices = img_slices
            pw = self.ws.get("b.pw", (slices * co * ckk,))
            pb = self.ws.get("b.pb", (slices * co,))
            if band_slices:
                check(lib.ssac_conv_first_wgrad_band(dy.data_ptr(), sv["img"].data_ptr(), pw.data_ptr(), pb.data_ptr(), B, ci,
                                                     Hi, Wi, co, k, s, self.div, self.shift, st))
            elif first:
                check(lib.ssac_conv_first_wgrad(dy.data_ptr(), sv["img"].data_ptr(), pw.data_ptr(), pb.data_ptr(), B, ci,
                                                Hi, Wi, co, k, s, self.div, self.shift, rps, st))
            elif img_slices:
                check(lib.ssac_conv_wgrad_img(dy.data_ptr(), sv["ys"][l - 1].data_ptr(), pw.data_ptr(), pb.data_ptr(), B, Hi,
                                              Wi, ci, co, k, s, st))
            elif self.implicit[l]:
                x_in = sv["ys"][l - 1]  # this layer's input = previous layer's ReLU output, channels-last
                check(lib.ssac_conv_wgrad(dy.data_ptr(), x_in.data_ptr(), pw.data_ptr(), pb.data_ptr(), B, Hi, Wi,
                                          ci, co, k, s, rps, st))
            else:
                check(lib.ssac_linear_wgrad_splitk(dy.data_ptr(), co, sv["cols"][l].data_ptr(), ckk, pw.data_ptr(),
                                                   pb.data_ptr(), co, ckk, rows, ROWS_PER_SLICE, st))
            check(lib.ssac_reduce_slices_pair(pw.data_ptr(), co * ckk, self._seg(2 * l, self.grads).data_ptr(),
                                              pb.data_ptr(), co, self._seg(2 * l + 1, self.grads).data_ptr(), slices, st))
            if l == 0:
                break
            pci, pco, pk, ps, pHi, pWi, pHo, pWo = sv["shapes"][l - 1]
            dprev = self.ws.get(f"b.dy{(l - 1) % 2}", (B * pHo * pWo * pco,))
            if self.implicit[l] and s <= 4:   # (strided layers: one parity class of input pixels per tile)
                check(lib.ssac_conv_dgrad(dy.data_ptr(), self.convs[l].weight.data_ptr(), sv["ys"][l - 1].data_ptr(),
                                          dprev.data_ptr(), B, Hi, Wi, ci, co, k, s, st))
            else:
                dcol = self.ws.get("b.dcol", (rows * ckk,))
                if ci % 4 == 0:
                    # columns in (ky, kx, c) order: the adjoint gather then reads 16 contiguous bytes per tap
                    wcl = self.ws.get("b.wcl", (co * ckk,))
                    check(lib.ssac_permute_cp(self.convs[l].weight.data_ptr(), wcl.data_ptr(), co, ci, k * k, 1, st))
                    check(lib.ssac_linear_dgrad(dy.data_ptr(), co, wcl.data_ptr(), ckk, dcol.data_ptr(), ckk, rows,
                                                ckk, co, st))
                    check(lib.ssac_col2im_cl(dcol.data_ptr(), dprev.data_ptr(), sv["ys"][l - 1].data_ptr(), B, ci, Hi,
                                             Wi, k, s, st))
                else:
                    check(lib.ssac_linear_dgrad(dy.data_ptr(), co, self.convs[l].weight.data_ptr(), ckk,
                                                dcol.data_ptr(), ckk, rows, ckk, co, st))
                    pcl = (pHo * pWo * pco, 1, pWo * pco, pco)
                    check(lib.ssac_col2im(dcol.data_ptr(), dprev.data_ptr(), *pcl, sv["ys"][l - 1].data_ptr(), *pcl,
                                          B, ci, Hi, Wi, k, s, st))
            dy = dprev


def conv_engine(encoder, device):
    """ConvEncoderEngine of `encoder` (cached on the wrapped conv module under encoder_base.cached_engine's rule), or None
    when it holds no convolutional module"""
    mod = find_conv_module(encoder)
    if mod is None:
        return None
    return cached_engine(mod, "_ssac_conv", device, lambda dev: ConvEncoderEngine(mod, dev))
