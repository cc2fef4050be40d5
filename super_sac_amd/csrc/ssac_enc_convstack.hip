// Plain two-layer convolution stacks on small maps (x / div + shift -> conv k1 (C -> 16) -> ReLU -> conv k2 (16 -> 16) ->
// ReLU -> NCHW flatten) on gfx950, exact fp32: the reference's MinAtar encoder (experiments/minatar/minatar_utils.py:37-63:
// 10 x 10 frames, 3 x 3 then 2 x 2 kernels, 16 channels) ahead of its fc, which stays on ssac_linear_fwd.
//
// Per layer such a stack runs on ssac_im2col + ssac_linear_fwd (conv_encoder.py); on 8 x 8 and 7 x 7 maps with 16 channels
// every one of those launches is latency-bound.  This file adds
//   ssac_enc_convstack_fwd   both convolutions in ONE launch: a workgroup (4 waves) owns a tile of SSAC_ENC_CONVSTACK_TILE = 4
//                            images, one wave per image.  The images are staged in LDS (the uint8 -> fp32 cast and
//                            x / div + shift in the staging loads), W1 and W2 beside them; each layer is an implicit GEMM on
//                            v_mfma_f32_16x16x4_f32 -- the 16 output channels are the A operand's rows, 16 output pixels the B
//                            operand's columns, K = C k k in steps of 4 (W1's rows zero-padded) -- with bias + ReLU in the
//                            epilogue.  The first map stays in LDS (and goes to H1 when asked for); the second map is
//                            written in NCHW flatten order, i.e. as the fc's input.
//   ssac_enc_convstack_bwd   from d(flat): dy2 = [h2 > 0] d(flat) -> LDS; dW2 (16 x 16 k2 k2) = sum over the tile's images
//                            and pixels of dy2 (x) patches(h1); layer 2's backward-data into LDS, masked by [h1 > 0], in
//                            place of h1; dW1 (16 x C k1 k1) likewise from the staged images; the bias gradients as row sums.
//                            ONE partial per workgroup, [dW1 | db1 | dW2 | db2] -- the layout of the parameter arena --
//                            for ssac_reduce_slices (fixed order).  Layer 1 has no backward-data.
// No atomics: every output has one owner and every sum a fixed order, so a replay is bit-identical.
//
// Index tables in LDS take the divisions out of the K loops: koff[k] is the offset of tap k = (c, ky, kx) from a patch's
// first element, pbase[p] the offset of output pixel p's patch in the input map.  A K pad (k >= K1) meets a zero weight
// and a finite staged value; a pixel pad (p >= P) reads a clamped address and is not stored (forward) or carries a zero
// A operand (weight gradients).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssac_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int R = SSAC_ENC_CONVSTACK_TILE;   // images per workgroup = waves per workgroup
constexpr int CO = 16;                       // output channels of both layers = rows of one MFMA tile
constexpr int MAX_LDS = 64 * 1024;           // the dynamic LDS a launch asks for, at most (no limit is raised)
constexpr int MAX_SIDE = 32, MAX_K = 4, MAX_C = 16, MAX_B = 1 << 22;

struct Geo {
    int B, C, H, W, k1, k2;
    int Wo1, P1, Wo2, Ho2, P2;   // output maps: P = Ho * Wo pixels
    int K1, K1p, K2;             // C k1 k1 (and rounded up to 4), 16 k2 k2
};

__host__ __device__ inline int fwd_lds_bytes(const Geo &g) {
    return 4 * (R * g.C * g.H * g.W + CO * (g.K1p + 1) + CO * (g.K2 + 1) + R * CO * g.P1 + 2 * CO + g.K1p + g.K2);
}
__host__ __device__ inline int bwd_lds_bytes(const Geo &g) {
    return 4 * (R * g.C * g.H * g.W + R * CO * g.P1 + R * CO * g.P2 + CO * g.K2 + g.K1p + 2 * g.K2 + g.P1 + g.P2);
}

bool make_geo(int B, int C, int H, int W, int co1, int k1, int s1, int co2, int k2, int s2, Geo *out) {
    if (co1 != CO || co2 != CO || s1 != 1 || s2 != 1 || C < 1 || C > MAX_C || k1 < 1 || k1 > MAX_K || k2 < 1 || k2 > MAX_K)
        return false;
    if (H > MAX_SIDE || W > MAX_SIDE || H < k1 + k2 - 1 || W < k1 + k2 - 1 || B < 1 || B > MAX_B) return false;
    Geo g;
    g.B = B; g.C = C; g.H = H; g.W = W; g.k1 = k1; g.k2 = k2;
    const int Ho1 = H - k1 + 1;
    g.Wo1 = W - k1 + 1; g.P1 = Ho1 * g.Wo1;
    g.Ho2 = Ho1 - k2 + 1; g.Wo2 = g.Wo1 - k2 + 1; g.P2 = g.Ho2 * g.Wo2;
    g.K1 = C * k1 * k1; g.K1p = (g.K1 + 3) / 4 * 4; g.K2 = CO * k2 * k2;
    if (fwd_lds_bytes(g) > MAX_LDS || bwd_lds_bytes(g) > MAX_LDS) return false;
    *out = g;
    return true;
}

__device__ __forceinline__ f32x4 zero4() {
    f32x4 z;
    z[0] = z[1] = z[2] = z[3] = 0.0f;
    return z;
}

// the tile's images, normalised, into LDS (zeros behind the batch's end)
__device__ __forceinline__ void stage_images(float *Xs, const void *X, int u8, float div, float shift, int img0, const Geo &g,
                                             int tid) {
    const int CHW = g.C * g.H * g.W;
    const bool plain = div == 1.0f && shift == 0.0f;
    for (int i = tid; i < R * CHW; i += 256) {
        const int r = i / CHW, img = img0 + r;
        float v = 0.0f;
        if (img < g.B) {
            const int64_t o = (int64_t)img * CHW + (i - r * CHW);
            const float x = u8 ? (float)static_cast<const uint8_t *>(X)[o] : static_cast<const float *>(X)[o];
            v = plain ? x : x / div + shift;
        }
        Xs[i] = v;
    }
}

// koff[k] for taps k = (c, ky, kx) of a k x k kernel over a map with `plane` elements per channel and rows of `width`
__device__ __forceinline__ void tap_offsets(int *koff, int n, int n_valid, int k, int plane, int width, int tid) {
    const int kk = k * k;
    for (int i = tid; i < n; i += 256) {
        const int c = i / kk, rem = i - c * kk, ky = rem / k, kx = rem - ky * k;
        koff[i] = i < n_valid ? c * plane + ky * width + kx : 0;
    }
}

// one layer of the forward for one image: OUT (16 x P, channel-major) = relu(Wt (16 x K, row stride ldw) . patches + bias)
template <bool TO_LDS>
__device__ __forceinline__ void conv_layer(const float *__restrict__ in, int in_width, const float *__restrict__ Wt, int ldw,
                                           int Kp, const int *__restrict__ koff, const float *__restrict__ bias, int Wo,
                                           int P, float *out_lds, float *out_mem, int lane) {
    const int col = lane & 15, kq = lane >> 4;
    const int tiles = (P + 15) >> 4;
    for (int t0 = 0; t0 < tiles; t0 += 4) {
        f32x4 acc[4];
        int base[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            acc[a] = zero4();
            const int p = min((t0 + a) * 16 + col, P - 1);
            const int oy = p / Wo;
            base[a] = oy * in_width + (p - oy * Wo);
        }
        for (int k0 = 0; k0 < Kp; k0 += 4) {
            const float w = Wt[col * ldw + k0 + kq];
            const int off = koff[k0 + kq];
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (t0 + a < tiles) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, in[base[a] + off], acc[a], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int p = (t0 + a) * 16 + col;
            if (t0 + a < tiles && p < P) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = kq * 4 + r;
                    const float v = fmaxf(acc[a][r] + bias[ch], 0.0f);
                    if (TO_LDS) out_lds[ch * P + p] = v;
                    if (out_mem) out_mem[ch * P + p] = v;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void convstack_fwd_kernel(const void *__restrict__ X, int u8, const float *__restrict__ W1,
                                                            const float *__restrict__ b1, const float *__restrict__ W2,
                                                            const float *__restrict__ b2, float div, float shift,
                                                            float *__restrict__ H1_save, float *__restrict__ OUT, Geo g) {
    extern __shared__ float lds[];
    const int CHW = g.C * g.H * g.W, ldw1 = g.K1p + 1, ldw2 = g.K2 + 1;
    float *Xs = lds, *W1s = Xs + R * CHW, *W2s = W1s + CO * ldw1, *H1s = W2s + CO * ldw2, *bs = H1s + R * CO * g.P1;
    int *koff1 = reinterpret_cast<int *>(bs + 2 * CO), *koff2 = koff1 + g.K1p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img0 = blockIdx.x * R;

    stage_images(Xs, X, u8, div, shift, img0, g, tid);
    for (int i = tid; i < CO * g.K1p; i += 256) {
        const int ch = i / g.K1p, k = i - ch * g.K1p;
        W1s[ch * ldw1 + k] = k < g.K1 ? W1[ch * g.K1 + k] : 0.0f;
    }
    for (int i = tid; i < CO * g.K2; i += 256) {
        const int ch = i / g.K2, k = i - ch * g.K2;
        W2s[ch * ldw2 + k] = W2[i];
    }
    if (tid < CO) bs[tid] = b1[tid];
    else if (tid < 2 * CO) bs[tid] = b2[tid - CO];
    tap_offsets(koff1, g.K1p, g.K1, g.k1, g.H * g.W, g.W, tid);
    tap_offsets(koff2, g.K2, g.K2, g.k2, g.P1, g.Wo1, tid);
    __syncthreads();

    // every wave runs both layers (a wave behind the batch's end works on zeros and stores nothing): the barriers are uniform
    const int img = img0 + wave;
    const bool live = img < g.B;
    float *h1 = H1s + wave * CO * g.P1;
    conv_layer<true>(Xs + wave * CHW, g.W, W1s, ldw1, g.K1p, koff1, bs, g.Wo1, g.P1, h1,
                     live && H1_save ? H1_save + (int64_t)img * CO * g.P1 : nullptr, lane);
    __syncthreads();
    if (live)   // (wave-uniform)
        conv_layer<false>(h1, g.Wo1, W2s, ldw2, g.K2, koff2, bs + CO, g.Wo2, g.P2, nullptr, OUT + (int64_t)img * CO * g.P2, lane);
}

// a weight gradient of the tile: G (16 x ncols) = sum over images r and output pixels p of dy[r][ch][p] * in[r][koff[j] +
// pbase[p]]; wave w owns the column tiles w, w + 4, ...  One accumulator per image (independent MFMA chains, and sums of
// at most P terms each), added as (0 + 1) + (2 + 3).
__device__ __forceinline__ void wgrad_tile(const float *__restrict__ dy, int P, const float *__restrict__ in, int in_size,
                                           const int *__restrict__ koff, const int *__restrict__ pbase, int ncols,
                                           float *__restrict__ G, int wave, int lane) {
    static_assert(R == 4, "one accumulator per image, summed pairwise");
    const int col = lane & 15, kq = lane >> 4;
    for (int tc = wave; tc * 16 < ncols; tc += 4) {
        const int j = tc * 16 + col;
        const float *x = in + koff[min(j, ncols - 1)];   // B: column = tap j
        const float *d = dy + col * P;                   // A: row = output channel `col`
        f32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = zero4();
        for (int p0 = 0; p0 < P; p0 += 4) {
            const int p = p0 + kq, pc = min(p, P - 1), pb = pbase[pc];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float a = p < P ? d[r * CO * P + pc] : 0.0f;
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[r * in_size + pb], acc[r], 0, 0, 0);
            }
        }
        if (j < ncols) {
#pragma unroll
            for (int q = 0; q < 4; ++q) G[(kq * 4 + q) * ncols + j] = (acc[0][q] + acc[1][q]) + (acc[2][q] + acc[3][q]);
        }
    }
}

// bias gradient: row sums of dy over the tile's images and pixels.  16 lanes per channel take every 16th pixel each, then
// a butterfly over the 16 lanes: a fixed tree, short chains
__device__ __forceinline__ void bias_grad(const float *__restrict__ dy, int P, float *__restrict__ G, int tid) {
    const int ch = tid >> 4, part = tid & 15;
    float s = 0.0f;
    for (int r = 0; r < R; ++r)
        for (int p = part; p < P; p += 16) s += dy[r * CO * P + ch * P + p];
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 16);
    if (part == 0) G[ch] = s;
}

__global__ __launch_bounds__(256) void convstack_bwd_kernel(const float *__restrict__ dFlat, const void *__restrict__ X, int u8,
                                                            float div, float shift, const float *__restrict__ H1,
                                                            const float *__restrict__ H2, const float *__restrict__ W2,
                                                            float *__restrict__ partial, Geo g) {
    extern __shared__ float lds[];
    const int CHW = g.C * g.H * g.W, kk2 = g.k2 * g.k2;
    float *Xs = lds, *H1s = Xs + R * CHW, *D2s = H1s + R * CO * g.P1, *W2s = D2s + R * CO * g.P2;
    int *koff1 = reinterpret_cast<int *>(W2s + CO * g.K2), *koff2 = koff1 + g.K1p, *kdec2 = koff2 + g.K2, *pbase1 = kdec2 + g.K2,
        *pbase2 = pbase1 + g.P1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4;
    const int img0 = blockIdx.x * R;
    float *out = partial + (int64_t)blockIdx.x * CO * (g.K1 + g.K2 + 2);
    float *gW1 = out, *gb1 = gW1 + CO * g.K1, *gW2 = gb1 + CO, *gb2 = gW2 + CO * g.K2;

    stage_images(Xs, X, u8, div, shift, img0, g, tid);
    for (int i = tid; i < R * CO * g.P1; i += 256) {
        const int r = i / (CO * g.P1), img = img0 + r;
        H1s[i] = img < g.B ? H1[(int64_t)img * CO * g.P1 + (i - r * CO * g.P1)] : 0.0f;
    }
    for (int i = tid; i < R * CO * g.P2; i += 256) {
        const int r = i / (CO * g.P2), img = img0 + r;
        float v = 0.0f;
        if (img < g.B) {
            const int64_t o = (int64_t)img * CO * g.P2 + (i - r * CO * g.P2);
            v = H2[o] > 0.0f ? dFlat[o] : 0.0f;
        }
        D2s[i] = v;
    }
    for (int i = tid; i < CO * g.K2; i += 256) W2s[i] = W2[i];
    tap_offsets(koff1, g.K1p, g.K1, g.k1, g.H * g.W, g.W, tid);
    tap_offsets(koff2, g.K2, g.K2, g.k2, g.P1, g.Wo1, tid);
    for (int i = tid; i < g.K2; i += 256) {   // k = (co2, ky, kx) of layer 2's backward-data
        const int co = i / kk2, rem = i - co * kk2, ky = rem / g.k2;
        kdec2[i] = (co << 16) | (ky << 8) | (rem - ky * g.k2);
    }
    for (int i = tid; i < g.P1; i += 256) pbase1[i] = (i / g.Wo1) * g.W + i % g.Wo1;
    for (int i = tid; i < g.P2; i += 256) pbase2[i] = (i / g.Wo2) * g.Wo1 + i % g.Wo2;
    __syncthreads();

    // ---- layer 2's weight and bias gradient (reads h1)
    wgrad_tile(D2s, g.P2, H1s, CO * g.P1, koff2, pbase2, g.K2, gW2, wave, lane);
    bias_grad(D2s, g.P2, gb2, tid);
    __syncthreads();

    // ---- layer 2's backward-data, masked, in place of h1: dy1[c1][y][x] = [h1 > 0] sum over (co2, ky, kx) of
    //      W2[co2][c1][ky][kx] * dy2[co2][y - ky][x - kx]; wave w owns the pixel tiles w, w + 4, ... of every image
    const int tiles1 = (g.P1 + 15) >> 4;
    for (int r = 0; r < R; ++r) {
        const float *d2 = D2s + r * CO * g.P2;
        float *h1 = H1s + r * CO * g.P1;
        for (int t = wave; t < tiles1; t += 4) {
            const int p = t * 16 + col, pc = min(p, g.P1 - 1);
            const int y = pc / g.Wo1, x = pc - y * g.Wo1;
            f32x4 acc = zero4();
            for (int k0 = 0; k0 < g.K2; k0 += 4) {
                const int k = k0 + kq, dec = kdec2[k];
                const int co = dec >> 16, ky = (dec >> 8) & 255, kx = dec & 255;
                const float w = W2s[co * g.K2 + col * kk2 + (k - co * kk2)];   // A: row = input channel `col` of layer 2
                const int yy = y - ky, xx = x - kx;
                const bool ok = p < g.P1 && yy >= 0 && yy < g.Ho2 && xx >= 0 && xx < g.Wo2;
                const float d = ok ? d2[co * g.P2 + yy * g.Wo2 + xx] : 0.0f;   // B: column = pixel `col` of the tile
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w, d, acc, 0, 0, 0);
            }
            if (p < g.P1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float *h = h1 + (kq * 4 + q) * g.P1 + p;
                    *h = *h > 0.0f ? acc[q] : 0.0f;
                }
            }
        }
    }
    __syncthreads();

    // ---- layer 1's weight and bias gradient
    wgrad_tile(H1s, g.P1, Xs, CHW, koff1, pbase1, g.K1, gW1, wave, lane);
    bias_grad(H1s, g.P1, gb1, tid);
}

}  // namespace

extern "C" int ssac_enc_convstack_covered(int C, int H, int W, int co1, int k1, int s1, int co2, int k2, int s2) {
    Geo g;
    return make_geo(1, C, H, W, co1, k1, s1, co2, k2, s2, &g) ? 1 : 0;
}

extern "C" int ssac_enc_convstack_supported(int B, int C, int H, int W, int co1, int k1, int s1, int co2, int k2, int s2) {
    // the shapes the fused form is the DEFAULT for: those it measured faster at than the per-layer launches by more than the
    // two ranges' overlap (profiles/conv_stack_encoder.md): MinAtar's geometry -- 10 x 10 frames, 3 x 3 then 2 x 2 kernels --
    // between the measured corners C 1 .. 16, B 1 .. 1024 (forward 18 .. 37 against 32 .. 74 us; backward 48 .. 96 against
    // 120 .. 270 us from B 32 on -- at B 1 the fused BACKWARD loses, 54 against 41 us at C 16, so the caller keeps passes that
    // are followed by a backward per layer below B 32: conv_encoder.STACK_BWD_MIN_ROWS).  Not measured counts as not
    // faster: every other covered geometry stays per layer.
    Geo g;
    if (!make_geo(B, C, H, W, co1, k1, s1, co2, k2, s2, &g)) return 0;
    return H == 10 && W == 10 && k1 == 3 && k2 == 2 && B <= 1024 ? 1 : 0;
}

extern "C" int ssac_enc_convstack_fwd(const void *X, int u8, const float *W1, const float *b1, const float *W2,
                                      const float *b2, int B, int C, int H, int W, int co1, int k1, int s1, int co2, int k2,
                                      int s2, float div, float shift, float *H1_save, float *out, void *stream) {
    Geo g;
    if (!make_geo(B, C, H, W, co1, k1, s1, co2, k2, s2, &g))
        return ssac_fail("ssac_enc_convstack_fwd: geometry not covered (see ssac_enc_convstack_covered)");
    if (!X || !W1 || !b1 || !W2 || !b2 || !out || div == 0.0f) return ssac_fail("ssac_enc_convstack_fwd: bad argument");
    SSAC_LAUNCH(convstack_fwd_kernel, dim3((B + R - 1) / R), dim3(256), (size_t)fwd_lds_bytes(g), (hipStream_t)stream, X, u8,
                W1, b1, W2, b2, div, shift, H1_save, out, g);
    return ssac_check_launch("enc_convstack_fwd");
}

extern "C" int ssac_enc_convstack_bwd(const float *d_flat, const void *X, int u8, const float *H1, const float *H2,
                                      const float *W2, int B, int C, int H, int W, int co1, int k1, int s1, int co2, int k2,
                                      int s2, float div, float shift, float *partial, void *stream) {
    Geo g;
    if (!make_geo(B, C, H, W, co1, k1, s1, co2, k2, s2, &g))
        return ssac_fail("ssac_enc_convstack_bwd: geometry not covered (see ssac_enc_convstack_covered)");
    if (!d_flat || !X || !H1 || !H2 || !W2 || !partial || div == 0.0f) return ssac_fail("ssac_enc_convstack_bwd: bad argument");
    SSAC_LAUNCH(convstack_bwd_kernel, dim3((B + R - 1) / R), dim3(256), (size_t)bwd_lds_bytes(g), (hipStream_t)stream, d_flat, X,
                u8, div, shift, H1, H2, W2, partial, g);
    return ssac_check_launch("enc_convstack_bwd");
}
