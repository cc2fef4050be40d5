// Colour augmentations on gfx950: ssac_aug_colour_jitter (ColorJitterAug, reference augmentations.py:537-771) and
// ssac_aug_netrand (NetworkRandomizationAug, augmentations.py:774-801).
//
// Neither fits the op table of ssac_aug_chain (ssac_aug.hip): colour jitter needs the mean of every (image, channel) plane,
// taken before or after an HSV round trip, and network randomisation is a 3 -> 3 channel 3 x 3 convolution.  Both work on
// groups of three channels, so ONE WORKGROUP HANDLES ONE (row, group): the three source planes are staged in LDS in the
// source's own type with 16-byte loads (gather through idx + uint8 -> fp32 fused, as in ssac_aug_chain), every pixel is
// evaluated from LDS, and the output is written once, 16 bytes per lane where the shape allows.
//
// Jitter runs two sweeps over the staged planes and RECOMPUTES instead of keeping fp32 intermediates: sweep 1 evaluates the
// stage in front of the contrast (nothing, or the HSV block) and sums the three planes; the sums are reduced in a fixed order
// (per-thread in pixel order, a shuffle tree per wave, the four waves in index order -- no atomics, so two launches are
// bit-equal and a uint8 and an fp32 source of the same values give the same bits); sweep 2 evaluates again, applies the
// contrast at its place and stores.  All arithmetic is fp32 in the reference's operation order, contraction off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssac_hip.h"
#include "ssac_internal.h"

namespace {

constexpr int COL_THREADS = 256;

// x / 255 of a staged element: a uint8 source goes through a 256-entry table of the correctly rounded quotients (the same
// bits as dividing), an fp32 source divides
template <typename T>
__device__ __forceinline__ float unit_of(T v, const float *lut) {
    if (sizeof(T) == 1) return lut[(int)v];
    return __fdiv_rn((float)v, 255.0f);
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// rgb2hsv -> adjust_brightness -> adjust_hue -> adjust_saturate -> hsv2rgb (augmentations.py:597-633, 693-771) of one pixel.
// shift = (fh * 255) / 360, evaluated once per row.  The floor-mods are written out for the ranges they meet, each with the
// rounding of torch's remainder (fmod, then + divisor where the result is negative):
//   a % 6 with |a| <= 1 (|g - b| <= delta):  a < 0 ? a + 6 : a
//   h % 1:                                   h - floor(h)   (exact for h >= 0; one rounding of h + k for h < 0, as torch's)
//   t % 2 with t >= 0:                       t - 2 floor(t / 2)   (exact)
__device__ __forceinline__ void hsv_block(float &r, float &g, float &b, float shift, float fb, float fs) {
#pragma clang fp contract(off)
    const float cmax = fmaxf(r, fmaxf(g, b)), cmin = fminf(r, fminf(g, b));
    const float delta = cmax - cmin;
    const float de = delta + 1e-8f;
    float hue = 0.0f;
    // assigned for Cmax == r, then == g, then == b: on ties b wins over g over r
    if (cmax == r) { const float a = __fdiv_rn(g - b, de); hue = a < 0.0f ? a + 6.0f : a; }
    if (cmax == g) hue = __fdiv_rn(b - r, de) + 2.0f;
    if (cmax == b) hue = __fdiv_rn(r - g, de) + 4.0f;
    if (cmax == 0.0f) hue = 0.0f;
    hue = __fdiv_rn(hue, 6.0f);
    float sat = __fdiv_rn(delta, cmax + 1e-8f);
    if (cmax == 0.0f) sat = 0.0f;
    float val = cmax;
    // brightness: v = clamp(v * fb), then everything clamped
    val = clamp01(val * fb);
    hue = clamp01(hue); sat = clamp01(sat);
    // hue
    hue = hue + shift;
    hue = hue - floorf(hue);
    // saturation
    sat = clamp01(sat * fs);
    hue = clamp01(hue); val = clamp01(val);
    // hsv2rgb
    const float hd = hue * 360.0f;
    const float ch = val * sat;
    const float t = __fdiv_rn(hd, 60.0f);
    const float t2 = t - 2.0f * floorf(t * 0.5f);
    const float x = -ch * (fabsf(t2 - 1.0f) - 1.0f);
    const float m = val - ch;
    float rp = 0.0f, gp = 0.0f, bp = 0.0f;   // a hue of exactly 360 matches no sector: (m, m, m)
    if (hd >= 0.0f && hd < 60.0f) { rp = ch; gp = x; }
    else if (hd >= 60.0f && hd < 120.0f) { rp = x; gp = ch; }
    else if (hd >= 120.0f && hd < 180.0f) { gp = ch; bp = x; }
    else if (hd >= 180.0f && hd < 240.0f) { gp = x; bp = ch; }
    else if (hd >= 240.0f && hd < 300.0f) { bp = ch; rp = x; }
    else if (hd >= 300.0f && hd < 360.0f) { bp = x; rp = ch; }
    r = clamp01(rp + m); g = clamp01(gp + m); b = clamp01(bp + m);
}

__device__ __forceinline__ float contrast_apply(float x, float mean, float fc) {
#pragma clang fp contract(off)
    return clamp01((x - mean) * fc + mean);
}

// the workgroup's share of a row: group g's three planes, and with the last group (or alone, c < 3) the leftover channels
struct Share {
    int ch0, n_main, n_left;   // channels [ch0, ch0 + n_main) are the group, the n_left behind them are leftovers
};
__device__ __forceinline__ Share share_of(int g, int c) {
    const int G = c / 3;
    Share s;
    s.ch0 = 3 * g;
    s.n_main = G > 0 ? 3 : 0;
    s.n_left = (G == 0 || g == G - 1) ? c - 3 * G : 0;
    return s;
}

// gather + convert of `count` contiguous elements (rows behind n_aug)
template <typename T>
__device__ __forceinline__ void plain_copy(const T *__restrict__ img, float *__restrict__ out, int count, int tid) {
    if ((count & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)img & (4 * sizeof(T) - 1)) == 0) {
        for (int i = tid; i < (count >> 2); i += COL_THREADS) {
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
        for (int i = tid; i < count; i += COL_THREADS) out[i] = (float)img[i];
    }
}

// leftover channels of an augmented row: x / 255 * 255 in fp32, straight from memory
template <typename T>
__device__ __forceinline__ void round_trip(const T *__restrict__ img, float *__restrict__ out, int count, int tid) {
#pragma clang fp contract(off)
    for (int i = tid; i < count; i += COL_THREADS) out[i] = __fmul_rn(__fdiv_rn((float)img[i], 255.0f), 255.0f);
}

// the group's three planes into LDS, 16 bytes per lane where the planes allow it
template <typename T>
__device__ __forceinline__ void stage_planes(const T *__restrict__ img, unsigned char *plane_raw, int hw, int tid) {
    const int bytes = 3 * hw * (int)sizeof(T);
    if ((bytes & 15) == 0 && ((uintptr_t)img & 15) == 0) {
        const uint4 *gsrc = reinterpret_cast<const uint4 *>(img);
        uint4 *l = reinterpret_cast<uint4 *>(plane_raw);
        for (int i = tid; i < (bytes >> 4); i += COL_THREADS) l[i] = gsrc[i];
    } else {
        T *pl = reinterpret_cast<T *>(plane_raw);
        for (int i = tid; i < 3 * hw; i += COL_THREADS) pl[i] = img[i];
    }
}

// PER (1 or 4) adjacent elements of one staged plane as x / 255; PER == 4 needs i0 % 4 == 0 and hw % 4 == 0
template <typename T, int PER>
__device__ __forceinline__ void load_units(const T *pl, int i0, const float *lut, float *x) {
    if (PER == 4) {
        if (sizeof(T) == 1) {
            const uint32_t u = *reinterpret_cast<const uint32_t *>(pl + i0);
            x[0] = lut[u & 255u]; x[1] = lut[(u >> 8) & 255u]; x[2] = lut[(u >> 16) & 255u]; x[3] = lut[u >> 24];
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(pl + i0);
            x[0] = __fdiv_rn(v.x, 255.0f); x[1] = __fdiv_rn(v.y, 255.0f);
            x[2] = __fdiv_rn(v.z, 255.0f); x[3] = __fdiv_rn(v.w, 255.0f);
        }
    } else {
        x[0] = unit_of(pl[i0], lut);
    }
}

template <int PER>
__device__ __forceinline__ void store_out(float *out, int i0, const float *v, bool aligned) {
    if (PER == 4 && aligned) {
        *reinterpret_cast<float4 *>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < PER; ++e) out[i0 + e] = v[e];
    }
}

struct JitterRow {
    float fc, shift, fb, fs;
};

// both sweeps of one (row, group).  Sweep 2 re-evaluates exactly what sweep 1 summed.
template <typename T, int PER>
__device__ __forceinline__ void jitter_sweeps(const T *pl, const float *lut, float *red, int hw, bool contrast_first,
                                              const JitterRow &jr, float *out, int tid) {
#pragma clang fp contract(off)
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int i0 = tid * PER; i0 < hw; i0 += COL_THREADS * PER) {
        float r[PER], g[PER], b[PER];
        load_units<T, PER>(pl, i0, lut, r);
        load_units<T, PER>(pl + hw, i0, lut, g);
        load_units<T, PER>(pl + 2 * hw, i0, lut, b);
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (!contrast_first) hsv_block(r[e], g[e], b[e], jr.shift, jr.fb, jr.fs);
            s0 += r[e]; s1 += g[e]; s2 += b[e];
        }
    }
    // fixed-order reduction: shuffle tree inside each wave, then the four waves in index order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64);
    }
    static_assert(COL_THREADS == 256, "four waves");
    if ((tid & 63) == 0) { red[(tid >> 6) * 3 + 0] = s0; red[(tid >> 6) * 3 + 1] = s1; red[(tid >> 6) * 3 + 2] = s2; }
    __syncthreads();
    const float n = (float)hw;
    const float m0 = __fdiv_rn(((red[0] + red[3]) + red[6]) + red[9], n);
    const float m1 = __fdiv_rn(((red[1] + red[4]) + red[7]) + red[10], n);
    const float m2 = __fdiv_rn(((red[2] + red[5]) + red[8]) + red[11], n);
    const bool aligned = ((uintptr_t)out & 15) == 0;
    for (int i0 = tid * PER; i0 < hw; i0 += COL_THREADS * PER) {
        float r[PER], g[PER], b[PER];
        load_units<T, PER>(pl, i0, lut, r);
        load_units<T, PER>(pl + hw, i0, lut, g);
        load_units<T, PER>(pl + 2 * hw, i0, lut, b);
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (contrast_first) {
                r[e] = contrast_apply(r[e], m0, jr.fc); g[e] = contrast_apply(g[e], m1, jr.fc); b[e] = contrast_apply(b[e], m2, jr.fc);
                hsv_block(r[e], g[e], b[e], jr.shift, jr.fb, jr.fs);
            } else {
                hsv_block(r[e], g[e], b[e], jr.shift, jr.fb, jr.fs);
                r[e] = contrast_apply(r[e], m0, jr.fc); g[e] = contrast_apply(g[e], m1, jr.fc); b[e] = contrast_apply(b[e], m2, jr.fc);
            }
            r[e] = r[e] * 255.0f; g[e] = g[e] * 255.0f; b[e] = b[e] * 255.0f;
        }
        store_out<PER>(out, i0, r, aligned);
        store_out<PER>(out + hw, i0, g, aligned);
        store_out<PER>(out + 2 * hw, i0, b, aligned);
    }
}

template <typename T>
__global__ __launch_bounds__(COL_THREADS) void colour_jitter_kernel(const T *__restrict__ src, const int64_t *__restrict__ idx,
                                                                    int c, int hw, const float *__restrict__ factors,
                                                                    uint32_t contrast_first, int n_aug,
                                                                    float *__restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plane_raw[];   // [3][hw] in the source's type
    __shared__ float lut[256];
    __shared__ float red[12];
    const int groups = max(c / 3, 1);
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups, tid = threadIdx.x;
    const Share sh = share_of(g, c);
    const T *img = src + ((idx ? idx[b] : (int64_t)b) * c + sh.ch0) * (int64_t)hw;
    float *out = dst + ((int64_t)b * c + sh.ch0) * hw;
    if (b >= n_aug) {
        plain_copy(img, out, (sh.n_main + sh.n_left) * hw, tid);
        return;
    }
    if (sh.n_left > 0) round_trip(img + (int64_t)sh.n_main * hw, out + (int64_t)sh.n_main * hw, sh.n_left * hw, tid);
    if (sh.n_main == 0) return;
    stage_planes(img, plane_raw, hw, tid);
    if (sizeof(T) == 1) lut[tid] = __fdiv_rn((float)tid, 255.0f);
    JitterRow jr;
    {
#pragma clang fp contract(off)
        jr.fc = factors[b * 4 + 0];
        jr.shift = __fdiv_rn(__fmul_rn(factors[b * 4 + 1], 255.0f), 360.0f);
        jr.fb = factors[b * 4 + 2];
        jr.fs = factors[b * 4 + 3];
    }
    __syncthreads();
    const bool cf = (contrast_first >> g) & 1u;
    const T *pl = reinterpret_cast<const T *>(plane_raw);
    if ((hw & 3) == 0) jitter_sweeps<T, 4>(pl, lut, red, hw, cf, jr, out, tid);
    else jitter_sweeps<T, 1>(pl, lut, red, hw, cf, jr, out, tid);
}

// PER adjacent outputs of row y starting at column x0 (PER == 4: w % 4 == 0, x0 % 4 == 0), all three output channels: the 27
// taps in the order ci, ky, kx, one fused multiply-add each; taps outside the image are zeros
template <typename T, int PER>
__device__ __forceinline__ void netrand_pixels(const T *pl, const float *lut, const float *wt, int h, int w, int y, int x0,
                                               float (*acc)[PER]) {
    const int hw = h * w;
#pragma unroll
    for (int co = 0; co < 3; ++co)
#pragma unroll
        for (int e = 0; e < PER; ++e) acc[co][e] = 0.0f;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            float v[PER + 2];
            if (yy >= 0 && yy < h) {
                const T *row = pl + ci * hw + yy * w;
                v[0] = x0 > 0 ? unit_of(row[x0 - 1], lut) : 0.0f;
                load_units<T, PER>(row, x0, lut, v + 1);
                v[PER + 1] = x0 + PER < w ? unit_of(row[x0 + PER], lut) : 0.0f;
            } else {
#pragma unroll
                for (int e = 0; e < PER + 2; ++e) v[e] = 0.0f;
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int co = 0; co < 3; ++co)
#pragma unroll
                    for (int e = 0; e < PER; ++e) acc[co][e] = __fmaf_rn(wt[(co * 3 + ci) * 9 + ky * 3 + kx], v[e + kx], acc[co][e]);
        }
    }
}

template <typename T, int PER>
__device__ __forceinline__ void netrand_sweep(const T *pl, const float *lut, const float *wt, int h, int w, float *out, int tid) {
    const int hw = h * w;
    const bool aligned = ((uintptr_t)out & 15) == 0;
    for (int i0 = tid * PER; i0 < hw; i0 += COL_THREADS * PER) {
        const int y = i0 / w, x0 = i0 - y * w;
        float acc[3][PER];
        netrand_pixels<T, PER>(pl, lut, wt, h, w, y, x0, acc);
#pragma unroll
        for (int co = 0; co < 3; ++co) {
#pragma unroll
            for (int e = 0; e < PER; ++e) acc[co][e] = __fmul_rn(acc[co][e], 255.0f);
            store_out<PER>(out + co * hw, i0, acc[co], aligned);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(COL_THREADS) void netrand_kernel(const T *__restrict__ src, const int64_t *__restrict__ idx, int c,
                                                              int h, int w, const float *__restrict__ weight, int n_aug,
                                                              float *__restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plane_raw[];   // [3][h * w] in the source's type
    __shared__ float lut[256];
    __shared__ float wt[81];   // [co][ci][ky][kx]
    const int hw = h * w;
    const int groups = max(c / 3, 1);
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups, tid = threadIdx.x;
    const Share sh = share_of(g, c);
    const T *img = src + ((idx ? idx[b] : (int64_t)b) * c + sh.ch0) * (int64_t)hw;
    float *out = dst + ((int64_t)b * c + sh.ch0) * hw;
    if (b >= n_aug) {
        plain_copy(img, out, (sh.n_main + sh.n_left) * hw, tid);
        return;
    }
    if (sh.n_left > 0) round_trip(img + (int64_t)sh.n_main * hw, out + (int64_t)sh.n_main * hw, sh.n_left * hw, tid);
    if (sh.n_main == 0) return;
    stage_planes(img, plane_raw, hw, tid);
    if (sizeof(T) == 1) lut[tid] = __fdiv_rn((float)tid, 255.0f);
    if (tid < 81) wt[tid] = weight[tid];
    __syncthreads();
    const T *pl = reinterpret_cast<const T *>(plane_raw);
    if ((w & 3) == 0) netrand_sweep<T, 4>(pl, lut, wt, h, w, out, tid);
    else netrand_sweep<T, 1>(pl, lut, wt, h, w, out, tid);
}

// the refusals both entry points share, made before any HIP call; 0 = accepted, *lds = the dynamic LDS of the launch
int colour_args(const char *who, const void *src, int src_dtype, int n, int c, int h, int w, const void *param, int n_aug,
                const float *dst, size_t *lds) {
    char msg[160];
    const char *why = nullptr;
    if (!src || !dst || !param || n <= 0 || c <= 0 || h <= 0 || w <= 0 || n_aug < 0) why = "bad arguments";
    else if ((const void *)dst == src) why = "dst must not alias src";
    else if (src_dtype != 0 && src_dtype != 1) why = "unsupported src_dtype";
    else if (c / 3 > SSAC_AUG_COLOUR_MAX_GROUPS) why = "more than SSAC_AUG_COLOUR_MAX_GROUPS (32) groups of three channels";
    else if ((size_t)3 * h * w * (src_dtype == 1 ? 1 : 4) > (size_t)SSAC_AUG_COLOUR_LDS_BYTES)
        why = "three image planes do not fit the LDS staging (SSAC_AUG_COLOUR_LDS_BYTES, 96 KB)";
    else if ((int64_t)n * (c / 3 > 0 ? c / 3 : 1) > 0x7fffffff) why = "too many (row, group) pairs";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", who, why);
        return ssac_fail(msg);
    }
    *lds = ((size_t)3 * h * w * (src_dtype == 1 ? 1 : 4) + 15) & ~(size_t)15;
    return 0;
}

bool g_jitter_lds_raised = false, g_netrand_lds_raised = false;

}  // namespace

extern "C" int ssac_aug_colour_jitter(const void *src, int src_dtype, const int64_t *idx, int n, int c, int h, int w,
                                      const float *factors, uint32_t contrast_first, int n_aug, float *dst, void *stream) {
    size_t lds = 0;
    if (colour_args("ssac_aug_colour_jitter", src, src_dtype, n, c, h, w, factors, n_aug, dst, &lds)) return 1;
    if (ssac_raise_lds(g_jitter_lds_raised, SSAC_AUG_COLOUR_LDS_BYTES, "ssac_aug_colour_jitter", colour_jitter_kernel<uint8_t>,
                       colour_jitter_kernel<float>))
        return 1;
    const int groups = c / 3 > 0 ? c / 3 : 1;
    hipStream_t st = (hipStream_t)stream;
    if (src_dtype == 1)
        SSAC_LAUNCH(colour_jitter_kernel<uint8_t>, dim3(n * groups), dim3(COL_THREADS), lds, st, (const uint8_t *)src, idx, c,
                    h * w, factors, contrast_first, n_aug, dst);
    else
        SSAC_LAUNCH(colour_jitter_kernel<float>, dim3(n * groups), dim3(COL_THREADS), lds, st, (const float *)src, idx, c,
                    h * w, factors, contrast_first, n_aug, dst);
    return ssac_check_launch("aug_colour_jitter");
}

extern "C" int ssac_aug_netrand(const void *src, int src_dtype, const int64_t *idx, int n, int c, int h, int w,
                                const float *weight, int n_aug, float *dst, void *stream) {
    size_t lds = 0;
    if (colour_args("ssac_aug_netrand", src, src_dtype, n, c, h, w, weight, n_aug, dst, &lds)) return 1;
    if (ssac_raise_lds(g_netrand_lds_raised, SSAC_AUG_COLOUR_LDS_BYTES, "ssac_aug_netrand", netrand_kernel<uint8_t>,
                       netrand_kernel<float>))
        return 1;
    const int groups = c / 3 > 0 ? c / 3 : 1;
    hipStream_t st = (hipStream_t)stream;
    if (src_dtype == 1)
        SSAC_LAUNCH(netrand_kernel<uint8_t>, dim3(n * groups), dim3(COL_THREADS), lds, st, (const uint8_t *)src, idx, c, h, w,
                    weight, n_aug, dst);
    else
        SSAC_LAUNCH(netrand_kernel<float>, dim3(n * groups), dim3(COL_THREADS), lds, st, (const float *)src, idx, c, h, w,
                    weight, n_aug, dst);
    return ssac_check_launch("aug_netrand");
}
