// Chained image augmentations on gfx950: ssac_aug_chain (cutout, cutout-color, translate, flips, rotate, window, gamma;
// reference augmentations.py:83-126, 296-534).
//
// Every one of them is an index map (translate, flips, rotate), a fill (cutout boxes, the translate border, the outside of
// a window) or a pointwise function (gamma).  So a whole chain is evaluated PER OUTPUT PIXEL, walking the row's ops from the
// last one to the first: a geometric op maps the coordinate, a fill op ends the walk with a constant, and the gammas
// BEHIND the point where the walk ended are applied to the value afterwards, in forward order.  One pass over the pixels
// whatever the chain length: each source byte is read once (gather through idx + uint8 -> fp32 fused, as ssac_drq_shift
// does), each output written once.
//
// Byte work, no MFMA: one workgroup per (row, channel) plane, the source plane staged in LDS in its own type with 16-byte
// loads, four adjacent output pixels per thread and 16-byte stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssac_hip.h"
#include "ssac_internal.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_LDS_BYTES = 60 * 1024;   // the staged plane (h * w * sizeof(T)) has to fit beside the static tables (64 KB)

// GammaAug.__call__ (augmentations.py:417-421): x / 255 (correctly rounded fp32, as ATen divides), the power (fp64, rounded
// once to fp32), * 255, clamp.  A negative gamma sends a 0 pixel to inf and the clamp to 255, as the reference does.
__device__ __forceinline__ float gamma_apply(float v, float g) {
#pragma clang fp contract(off)
    const float x = __fdiv_rn(v, 255.0f);
    const float p = (float)pow((double)x, (double)g);
    return fminf(fmaxf(__fmul_rn(p, 255.0f), 0.0f), 255.0f);
}

// the gammas at positions > stop, in forward order (stop = -1: all of them)
__device__ __forceinline__ float gamma_tail(float v, const ssac_aug_op *ops, int n_ops, int stop) {
    for (int j = stop + 1; j < n_ops; ++j)
        if (ops[j].op == SSAC_AUG_GAMMA) v = gamma_apply(v, ops[j].f0);
    return v;
}

__device__ __forceinline__ float fill_colour(const ssac_aug_op &o, int ch) {
    const int k = ch % 3;
    return k == 0 ? o.f0 : (k == 1 ? o.f1 : o.f2);
}

template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void aug_chain_kernel(const T *__restrict__ src, const int64_t *__restrict__ idx,
                                                                int c, int h, int w, const ssac_aug_op *__restrict__ ops,
                                                                int ops_stride, int n_ops, int n_aug,
                                                                float *__restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plane_raw[];
    T *pl = reinterpret_cast<T *>(plane_raw);              // [h * w] the source plane, in the source's type
    __shared__ ssac_aug_op sops[SSAC_AUG_MAX_OPS];
    __shared__ float fillv[SSAC_AUG_MAX_OPS];               // value a walk that ends at op j writes (gammas behind j applied)
    __shared__ float lut[256];                              // uint8 source: byte -> value after every gamma of the row
    const int b = blockIdx.x / c, ch = blockIdx.x - b * c, tid = threadIdx.x;
    const int hw = h * w;
    const T *img = src + ((idx ? idx[b] : (int64_t)b) * c + ch) * (int64_t)hw;
    float *out = dst + ((int64_t)b * c + ch) * hw;
    const bool vec4 = (hw & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)img & (4 * sizeof(T) - 1)) == 0;

    // rows beyond the augmented part of the mix, and rows whose ops are all no-ops (a flip that was not drawn, a rotation
    // by 0 turns): gather + convert, straight from memory
    bool plain = b >= n_aug;
    if (!plain) {
        plain = true;
        for (int j = 0; j < n_ops; ++j) plain = plain && ops[(int64_t)b * ops_stride + j].op == SSAC_AUG_NOP;
    }
    if (plain) {
        if (vec4) {
            for (int i = tid; i < (hw >> 2); i += AUG_THREADS) {
                float4 v;
                if (sizeof(T) == 1) {
                    const uint32_t u = reinterpret_cast<const uint32_t *>(img)[i];
                    v = make_float4((float)(u & 255u), (float)((u >> 8) & 255u), (float)((u >> 16) & 255u), (float)(u >> 24));
                } else {
                    v = reinterpret_cast<const float4 *>(img)[i];
                }
                reinterpret_cast<float4 *>(out)[i] = v;
            }
        } else {
            for (int i = tid; i < hw; i += AUG_THREADS) out[i] = (float)img[i];
        }
        return;
    }

    // stage the plane: 16 bytes per lane where the plane allows it
    const int bytes = hw * (int)sizeof(T);
    if ((bytes & 15) == 0 && ((uintptr_t)img & 15) == 0) {
        const uint4 *g = reinterpret_cast<const uint4 *>(img);
        uint4 *l = reinterpret_cast<uint4 *>(plane_raw);
        for (int i = tid; i < (bytes >> 4); i += AUG_THREADS) l[i] = g[i];
    } else {
        for (int i = tid; i < hw; i += AUG_THREADS) pl[i] = img[i];
    }
    if (tid < n_ops * 8)   // (8 words per op, copied word by word)
        reinterpret_cast<int32_t *>(sops)[tid] = reinterpret_cast<const int32_t *>(ops + (int64_t)b * ops_stride)[tid];
    __syncthreads();
    bool has_gamma = false;
    for (int j = 0; j < n_ops; ++j) has_gamma = has_gamma || sops[j].op == SSAC_AUG_GAMMA;
    if (tid < n_ops) {
        const ssac_aug_op &o = sops[tid];
        float v = 0.0f;                                      // cutout box, outside of the window
        if (o.op == SSAC_AUG_TRANSLATE || o.op == SSAC_AUG_CUTOUT_COLOR) v = fill_colour(o, ch);
        fillv[tid] = has_gamma ? gamma_tail(v, sops, n_ops, tid) : v;
    }
    static_assert(AUG_THREADS == 256, "one thread per entry of the byte -> value table");
    if (sizeof(T) == 1 && has_gamma) lut[tid] = gamma_tail((float)tid, sops, n_ops, -1);
    __syncthreads();

    // A thread owns four adjacent output pixels (one without the 16-byte path) and walks the ops ONCE for all of them: an
    // op's operands are read from LDS once per op, made scalar (they are the same in every lane), and the kind of the op
    // is one scalar branch.  The two forms tried before this one are in profiles/aug_chain.md.
    const int c3 = 3 * (c / 3);   // CutoutColorAug paints whole RGB groups only (augmentations.py:377-382)
    const int per = vec4 ? 4 : 1;
    for (int i0 = tid * per; i0 < hw; i0 += AUG_THREADS * per) {
        int yy[4], xx[4], stop[4];
        {
            int y = i0 / w, x = i0 - y * w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                yy[e] = y; xx[e] = x; stop[e] = -1;
                if (e + 1 < per && ++x == w) { x = 0; ++y; }   // (per == 1: the other three repeat the pixel, unused)
            }
        }
        for (int j = n_ops - 1; j >= 0; --j) {
            const int op = __builtin_amdgcn_readfirstlane(sops[j].op);
            if (op == SSAC_AUG_NOP || op == SSAC_AUG_GAMMA) continue;   // (gamma: applied behind the walk)
            const int a0 = __builtin_amdgcn_readfirstlane(sops[j].i0), a1 = __builtin_amdgcn_readfirstlane(sops[j].i1);
            const int a2 = __builtin_amdgcn_readfirstlane(sops[j].i2), a3 = __builtin_amdgcn_readfirstlane(sops[j].i3);
            // a pixel whose walk has ended (stop >= 0) ignores the ops in front of the fill
#define AUG_EACH(BODY)                                                                       \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                          \
        int ny = yy[e], nx = xx[e];                                                          \
        bool fill = false;                                                                   \
        BODY;                                                                                \
        if (stop[e] < 0) { yy[e] = ny; xx[e] = nx; if (fill) stop[e] = j; }                  \
    }
            switch (op) {
            case SSAC_AUG_CUTOUT:         // i0..i3 = row0, row1, col0, col1 (half-open, clipped by the image)
                AUG_EACH(fill = ny >= a0 && ny < a1 && nx >= a2 && nx < a3)
                break;
            case SSAC_AUG_CUTOUT_COLOR:
                if (ch < c3) { AUG_EACH(fill = ny >= a0 && ny < a1 && nx >= a2 && nx < a3) }
                break;
            case SSAC_AUG_TRANSLATE:      // out[y, x] = in[y - i0, x - i1], the border in the row's colour
                AUG_EACH(ny -= a0; nx -= a1; fill = ny < 0 || ny >= h || nx < 0 || nx >= w)
                break;
            case SSAC_AUG_HFLIP: AUG_EACH(nx = w - 1 - nx) break;
            case SSAC_AUG_VFLIP: AUG_EACH(ny = h - 1 - ny) break;
            case SSAC_AUG_ROTATE:         // torch.rot90(k = i0, dims = (2, 3)); odd k on square planes only (host)
                if (a0 == 2) { AUG_EACH(ny = h - 1 - ny; nx = w - 1 - nx) }
                else if (a0 == 1) { AUG_EACH(const int t = ny; ny = nx; nx = w - 1 - t) }
                else if (a0 == 3) { AUG_EACH(const int t = ny; ny = h - 1 - nx; nx = t) }
                break;
            case SSAC_AUG_WINDOW:         // everything outside rows [i0, i0 + i2) x columns [i1, i1 + i2) is 0
                AUG_EACH(fill = ny < a0 || ny >= a0 + a2 || nx < a1 || nx >= a1 + a2)
                break;
            default: break;
            }
#undef AUG_EACH
        }
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v;
            if (stop[e] >= 0) {
                v = fillv[stop[e]];
            } else {
                // (in range by construction; the clamp keeps a malformed table inside the staged plane)
                const T p = pl[min(max(yy[e], 0), h - 1) * w + min(max(xx[e], 0), w - 1)];
                if (!has_gamma) v = (float)p;
                else if (sizeof(T) == 1) v = lut[(int)p];
                else v = gamma_tail((float)p, sops, n_ops, -1);
            }
            r[e] = v;
        }
        if (vec4) *reinterpret_cast<float4 *>(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
        else out[i0] = r[0];
    }
}

}  // namespace

extern "C" int ssac_aug_chain(const void *src, int src_dtype, const int64_t *idx, int n, int c, int h, int w,
                              const ssac_aug_op *ops, int ops_stride, int n_ops, int n_aug, float *dst, void *stream) {
    if (!src || !dst || n <= 0 || c <= 0 || h <= 0 || w <= 0) return ssac_fail("ssac_aug_chain: bad arguments");
    if (n_ops < 0 || n_ops > SSAC_AUG_MAX_OPS || ops_stride < n_ops || (n_ops > 0 && !ops))
        return ssac_fail("ssac_aug_chain: at most SSAC_AUG_MAX_OPS ops per row, ops_stride >= n_ops");
    if (src_dtype != 0 && src_dtype != 1) return ssac_fail("ssac_aug_chain: unsupported src_dtype");
    const size_t lds = (size_t)h * w * (src_dtype == 1 ? 1 : 4);
    if (lds > (size_t)AUG_LDS_BYTES) return ssac_fail("ssac_aug_chain: the image plane does not fit the LDS staging (60 KB)");
    if ((int64_t)n * c > 0x7fffffff) return ssac_fail("ssac_aug_chain: too many planes");
    if (n_ops == 0) n_aug = 0;
    hipStream_t st = (hipStream_t)stream;
    if (src_dtype == 1)
        SSAC_LAUNCH(aug_chain_kernel<uint8_t>, dim3(n * c), dim3(AUG_THREADS), (lds + 15) & ~(size_t)15, st,
                    (const uint8_t *)src, idx, c, h, w, ops, ops_stride, n_ops, n_aug, dst);
    else
        SSAC_LAUNCH(aug_chain_kernel<float>, dim3(n * c), dim3(AUG_THREADS), (lds + 15) & ~(size_t)15, st,
                    (const float *)src, idx, c, h, w, ops, ops_stride, n_ops, n_aug, dst);
    return ssac_check_launch("aug_chain");
}
