// Two-layer MLP encoders (obs -> Linear(K, H) -> ReLU -> Linear(H, N) -> act2) on gfx950, exact fp32.
//
// The reference's vector encoders (experiments/gym/train_gym.py SharedEncoder, experiments/visgrid/train.py
// VisgridEncoder) are two nn.Linear layers.  Per layer they run on ssac_linear_fwd / ssac_linear_dgrad_masked /
// ssac_linear_wgrad_splitk (ssac_gemm.hip); this file adds
//   ssac_enc_act_fwd / ssac_enc_act_bwd   the output activation (tanh) and act2'(y) * dy as elementwise passes, and
//   ssac_enc_mlp2_fwd / ssac_enc_mlp2_bwd both layers in ONE launch each: a workgroup owns 32 rows, the hidden tile
//                                         (32 x H) never leaves LDS between the two products.
// All products are v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per output element), bias and activation are separate
// fp32 operations (-ffp-contract=off), and no reduction uses atomics: every output element has one owner, so a replay
// is bit-identical.
//
// Forward, per workgroup (256 threads = 4 waves, row tile r0 .. r0 + 31):
//   phase 1  K in chunks of 32: X chunk (32 x 32) and W0 chunk (H x 32) staged through LDS with guarded scalar loads
//            (any K, any ldx, any alignment); wave w owns the hidden column blocks w and w + 4 (H <= 256: two
//            accumulators).  h = relu(acc + b0) goes to LDS (stride H + 1: the A-operand reads of phase 2 are
//            conflict free) and, when asked for, to H_save.
//   phase 2  wave w owns the output column blocks w, w + 4, ...: A operand from the hidden tile in LDS, B operand = the
//            wave's 32 rows of W1 read 16 bytes per lane straight from memory (rows of H floats, H % 32 == 0; lane half
//            h takes k + 4 h .. + 3 of every 8, as ssac_linear_fwd_stream does).  Columns past N read row N - 1 and are
//            not stored.
// Backward, per workgroup (same tile): N in chunks of 32: dZ1 = act2'(Y) * dY of the chunk is computed while it is staged
//            (and written out for the weight gradient), the W1 chunk (32 x H) is staged beside it; wave w accumulates
//            the hidden column blocks w and w + 4 of dZ1 W1; the epilogue applies [h > 0] from H_save.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssac_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int ROWS = 32;          // rows per workgroup = one MFMA tile
constexpr int XS = 33;            // LDS stride of a K-contiguous 32-wide chunk row: bank = (row + k) % 32
constexpr int MAX_H = 256;        // hidden width: two 32-column blocks per wave at most
constexpr int MAX_DIM = 1 << 20;  // K and N
constexpr int MAX_ROWS = 1 << 24; // M

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

__device__ __forceinline__ float act_fwd(float v, int act) {
    return act == ACT_RELU ? fmaxf(v, 0.0f) : act == ACT_TANH ? tanhf(v) : v;
}
// act'(.) from the activation's OUTPUT y
__device__ __forceinline__ float act_bwd(float y, float dy, int act) {
    if (act == ACT_RELU) return y > 0.0f ? dy : 0.0f;
    if (act == ACT_TANH) return (1.0f - y * y) * dy;
    return dy;
}

__global__ __launch_bounds__(256) void enc_act_fwd_kernel(float *__restrict__ Y, int64_t ldy, int M, int N, int act) {
    const int64_t total = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / N;
        float *p = Y + r * ldy + (i - r * N);
        *p = act_fwd(*p, act);
    }
}

__global__ __launch_bounds__(256) void enc_act_bwd_kernel(const float *__restrict__ dY, int64_t ldd,
                                                          const float *__restrict__ Y, int64_t ldy, int M, int N,
                                                          int act, float *__restrict__ dZ) {
    const int64_t total = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / N, c = i - r * N;
        dZ[i] = act_bwd(Y[r * ldy + c], dY[r * ldd + c], act);
    }
}

// dynamic LDS (floats): phase 1 holds Xs[32][33] | Ws[H][33]; phase 2 re-uses the area as Hs[32][H + 1]
__host__ __device__ constexpr int fwd_lds_floats(int H) {
    return (ROWS + H) * XS > ROWS * (H + 1) ? (ROWS + H) * XS : ROWS * (H + 1);
}

__global__ __launch_bounds__(256) void enc_mlp2_fwd_kernel(const float *__restrict__ X, int64_t ldx,
                                                           const float *__restrict__ W0, const float *__restrict__ b0,
                                                           const float *__restrict__ W1, const float *__restrict__ b1,
                                                           int M, int K, int H, int N, int act2,
                                                           float *__restrict__ H_save, float *__restrict__ Y, int64_t ldy) {
    extern __shared__ float lds[];
    float *Xs = lds, *Ws = lds + ROWS * XS, *Hs = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int r0 = blockIdx.x * ROWS;
    const int hblocks = H >> 5;
    const int kk = tid & 31, rr = tid >> 5;   // staging: thread -> column kk of rows rr, rr + 8, ...

    // ---- phase 1: h = relu(X W0^T + b0)
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 32) {
        const bool kok = k0 + kk < K;
#pragma unroll
        for (int p = 0; p < ROWS / 8; ++p) {
            const int row = r0 + rr + 8 * p;
            const bool ok = kok && row < M;
            const float v = X[ok ? (int64_t)row * ldx + k0 + kk : 0];
            Xs[(rr + 8 * p) * XS + kk] = ok ? v : 0.0f;
        }
        for (int p = 0; p < H / 8; ++p) {
            const int row = rr + 8 * p;
            const float v = W0[kok ? (int64_t)row * K + k0 + kk : 0];
            Ws[row * XS + kk] = kok ? v : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int cb = wave + 4 * a;
            if (cb < hblocks) {
                const float *xa = Xs + li * XS + lh, *wb = Ws + (cb * 32 + li) * XS + lh;
#pragma unroll
                for (int k = 0; k < 32; k += 2) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k], wb[k], acc[a], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // (the second barrier of the last chunk ordered every read of Xs / Ws before these writes of Hs)
    const int ldh = H + 1;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int cb = wave + 4 * a;
        if (cb < hblocks) {
            const int col = cb * 32 + li;
            const float bias = b0[col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float h = fmaxf(acc[a][r] + bias, 0.0f);
                Hs[row * ldh + col] = h;
                if (H_save && r0 + row < M) H_save[(int64_t)(r0 + row) * H + col] = h;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: Y = act2(h W1^T + b1)
    const int nblocks = (N + 31) >> 5;
    for (int nb = wave; nb < nblocks; nb += 4) {
        const int col = nb * 32 + li;
        const float4 *wrow = reinterpret_cast<const float4 *>(W1 + (int64_t)min(col, N - 1) * H + 4 * lh);
        const float *ha = Hs + li * ldh + 4 * lh;
        f32x16 out;
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = 0.0f;
        for (int k0 = 0; k0 < H; k0 += 32) {
            float4 w[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) w[g] = wrow[(k0 >> 2) + 2 * g];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float *hp = ha + k0 + 8 * g;
                out = __builtin_amdgcn_mfma_f32_32x32x2f32(hp[0], w[g].x, out, 0, 0, 0);
                out = __builtin_amdgcn_mfma_f32_32x32x2f32(hp[1], w[g].y, out, 0, 0, 0);
                out = __builtin_amdgcn_mfma_f32_32x32x2f32(hp[2], w[g].z, out, 0, 0, 0);
                out = __builtin_amdgcn_mfma_f32_32x32x2f32(hp[3], w[g].w, out, 0, 0, 0);
            }
        }
        if (col < N) {
            const float bias = b1[col];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < M) Y[(int64_t)row * ldy + col] = act_fwd(out[r] + bias, act2);
            }
        }
    }
}

// dynamic LDS (floats) of the backward: Ds[32][33] | Wt[32][H]
__host__ __device__ constexpr int bwd_lds_floats(int H) { return ROWS * XS + 32 * H; }

__global__ __launch_bounds__(256) void enc_mlp2_bwd_kernel(const float *__restrict__ dY, int64_t ldd,
                                                           const float *__restrict__ Y, int64_t ldy,
                                                           const float *__restrict__ H_save, const float *__restrict__ W1,
                                                           int M, int H, int N, int act2, float *__restrict__ dZ1,
                                                           float *__restrict__ dZ0) {
    extern __shared__ float lds[];
    float *Ds = lds, *Wt = lds + ROWS * XS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int r0 = blockIdx.x * ROWS;
    const int hblocks = H >> 5;
    const int kk = tid & 31, rr = tid >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
    for (int n0 = 0; n0 < N; n0 += 32) {
        // dZ1 chunk: column n0 + kk of rows rr + 8 p (zero outside the problem), kept for the weight gradient
        const bool nok = n0 + kk < N;
#pragma unroll
        for (int p = 0; p < ROWS / 8; ++p) {
            const int row = r0 + rr + 8 * p;
            const bool ok = nok && row < M;
            const float y = Y[ok ? (int64_t)row * ldy + n0 + kk : 0];
            const float d = dY[ok ? (int64_t)row * ldd + n0 + kk : 0];
            const float dz = ok ? act_bwd(y, d, act2) : 0.0f;
            Ds[(rr + 8 * p) * XS + kk] = dz;
            if (ok) dZ1[(int64_t)row * N + n0 + kk] = dz;
        }
        // W1 chunk: rows n0 .. n0 + 31 (zero past N), all H columns, read along the rows
        for (int i = tid; i < 32 * H; i += 256) {
            const int n = i / H, c = i - n * H;
            const bool ok = n0 + n < N;
            const float v = W1[ok ? (int64_t)(n0 + n) * H + c : 0];
            Wt[i] = ok ? v : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int cb = wave + 4 * a;
            if (cb < hblocks) {
                const float *da = Ds + li * XS + lh, *wb = Wt + lh * H + cb * 32 + li;
#pragma unroll
                for (int k = 0; k < 32; k += 2) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(da[k], wb[k * H], acc[a], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int cb = wave + 4 * a;
        if (cb < hblocks) {
            const int col = cb * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (row < M) {
                    const int64_t o = (int64_t)row * H + col;
                    dZ0[o] = H_save[o] > 0.0f ? acc[a][r] : 0.0f;
                }
            }
        }
    }
}

bool covered(int M, int K, int H, int N) {
    return M > 0 && M <= MAX_ROWS && K > 0 && K <= MAX_DIM && N > 0 && N <= MAX_DIM && H >= 32 && H <= MAX_H && (H & 31) == 0;
}

int elementwise_blocks(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace

extern "C" int ssac_enc_mlp2_covered(int M, int K, int H, int N) { return covered(M, K, H, N) ? 1 : 0; }

extern "C" int ssac_enc_mlp2_supported(int M, int K, int H, int N) {
    // the shapes the fused FORWARD is the default for: those it measured faster at than the two per-layer launches
    // (profiles/mlp_encoder.md: 17 -> 128 -> 17 at B 256 / 512, 9.3 against 13.3 us; at K 324 and 376 its unpipelined K loop
    // over 8 .. 16 workgroups lost, 37 .. 44 against 22 .. 27 us) -- one K chunk.  The fused backward won nowhere.
    return covered(M, K, H, N) && K <= 32 ? 1 : 0;
}

extern "C" int ssac_enc_act_fwd(float *Y, int64_t ldy, int M, int N, int act, void *stream) {
    if (M <= 0 || N <= 0 || ldy < N || act < ACT_NONE || act > ACT_TANH) return ssac_fail("ssac_enc_act_fwd: bad shape or activation");
    if (act == ACT_NONE) return 0;
    SSAC_LAUNCH(enc_act_fwd_kernel, dim3(elementwise_blocks((int64_t)M * N)), dim3(256), 0, (hipStream_t)stream, Y, ldy, M,
                N, act);
    return ssac_check_launch("enc_act_fwd");
}

extern "C" int ssac_enc_act_bwd(const float *dY, int64_t ldd, const float *Y, int64_t ldy, int M, int N, int act,
                                float *dZ, void *stream) {
    if (M <= 0 || N <= 0 || ldy < N || ldd < N || act < ACT_NONE || act > ACT_TANH)
        return ssac_fail("ssac_enc_act_bwd: bad shape or activation");
    SSAC_LAUNCH(enc_act_bwd_kernel, dim3(elementwise_blocks((int64_t)M * N)), dim3(256), 0, (hipStream_t)stream, dY, ldd, Y,
                ldy, M, N, act, dZ);
    return ssac_check_launch("enc_act_bwd");
}

extern "C" int ssac_enc_mlp2_fwd(const float *X, int64_t ldx, const float *W0, const float *b0, const float *W1,
                                 const float *b1, int M, int K, int H, int N, int act2, float *H_save, float *Y,
                                 int64_t ldy, void *stream) {
    if (!covered(M, K, H, N)) return ssac_fail("ssac_enc_mlp2_fwd: shape not covered (see ssac_enc_mlp2_covered)");
    if (ldx < K || ldy < N || act2 < ACT_NONE || act2 > ACT_TANH) return ssac_fail("ssac_enc_mlp2_fwd: bad stride or activation");
    if ((uintptr_t)W1 & 15) return ssac_fail("ssac_enc_mlp2_fwd: W1 must be 16-byte aligned");
    SSAC_LAUNCH(enc_mlp2_fwd_kernel, dim3((M + ROWS - 1) / ROWS), dim3(256), (size_t)fwd_lds_floats(H) * sizeof(float),
                (hipStream_t)stream, X, ldx, W0, b0, W1, b1, M, K, H, N, act2, H_save, Y, ldy);
    return ssac_check_launch("enc_mlp2_fwd");
}

extern "C" int ssac_enc_mlp2_bwd(const float *dY, int64_t ldd, const float *Y, int64_t ldy, const float *H_save,
                                 const float *W1, int M, int H, int N, int act2, float *dZ1, float *dZ0, void *stream) {
    if (!covered(M, 1, H, N)) return ssac_fail("ssac_enc_mlp2_bwd: shape not covered (see ssac_enc_mlp2_covered)");
    if (ldd < N || ldy < N || act2 < ACT_NONE || act2 > ACT_TANH) return ssac_fail("ssac_enc_mlp2_bwd: bad stride or activation");
    SSAC_LAUNCH(enc_mlp2_bwd_kernel, dim3((M + ROWS - 1) / ROWS), dim3(256), (size_t)bwd_lds_floats(H) * sizeof(float),
                (hipStream_t)stream, dY, ldd, Y, ldy, H_save, W1, M, H, N, act2, dZ1, dZ0);
    return ssac_check_launch("enc_mlp2_bwd");
}
