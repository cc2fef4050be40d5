// Two-layer MLP encoders (obs -> Linear(K, H) -> ReLU -> Linear(H, N) -> act2) on gfx950, exact fp32.
//
// The reference's vector encoders (experiments/gym/train_gym.py SharedEncoder, experiments/visgrid/train.py
// VisgridEncoder) are two nn.Linear layers.  Per layer they run on ssac_linear_fwd / ssac_linear_dgrad_masked /
// ssac_linear_wgrad_splitk (ssac_gemm.hip); this file adds
//   ssac_enc_act_fwd / ssac_enc_act_bwd   the output activation (tanh) and act2'(y) * dy as elementwise passes, and
//   ssac_enc_mlp2_fwd / ssac_enc_mlp2_bwd both layers in ONE launch each: a workgroup owns 32 rows, the hidden tile
//                                         (32 x H) never leaves LDS between the two products, and
//   ssac_enc_mlp2_fwd_rows                the forward of 1 .. 16 rows (an acting call) without a tile: fmaf chains, layer 1
//                                         spread over H / 4 workgroups, layer 2 by the last of them to arrive (see below).
// The tile launches' products are v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per output element), bias and activation
// are separate fp32 operations (-ffp-contract=off), and no reduction uses atomics (the few-row forward's one atomic counts
// arrivals, never data): every output element has one owner, so a replay is bit-identical.
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

// ---- the few-row forward (acting calls: 1 .. 16 rows) ------------------------------------------------------------------
// A GEMV-shaped, latency-bound problem: no MFMA tile, no LDS staging of the weights.  Layer 1 is spread over H / 4
// workgroups of 4 waves; a wave owns ONE hidden unit for all rows: its W0 row goes straight to VGPRs (16 bytes per lane
// where the row is aligned, guarded scalar loads otherwise -- the same k order either way), K is split over the 64 lanes
// (lane l takes k = 4 l .. 4 l + 3 of every 256), the rows of X come from a zero-padded LDS image, and the lanes' partial
// sums meet in a fixed xor-shuffle tree (32, 16, .. 1).  h = relu(sum + b0) goes to `hbuf` in global memory.
// Layer 2 is the work of the LAST workgroup to arrive: every thread fences its h stores, the workgroup's thread 0 adds 1
// to an arrival counter, and whoever reads gridDim.x - 1 back continues -- nobody waits for anybody, a workgroup that is not
// last simply ends.  The last one returns the counter to zero for the next launch, reads h (loads that bypass the
// vector cache) into LDS and computes Y: S lanes per output column (S a power of two fixed by N and H alone), lane s
// of a group takes the 16-byte chunks s, s + S, .. of its W1 row in ascending order, the group reduces by the same kind
// of tree.  Which workgroup arrives last changes who computes, never what is summed in which order: every output element
// has one owner and one summation order per (M, K, H, N) -- a replay is bit-identical.
constexpr int ROWS_MAX_M = 16;
constexpr int ROWS_MAX_K = 512;       // the X image: 16 rows x 512 floats = 32 KiB of LDS
constexpr int ROWS_MAX_N = 1 << 16;
constexpr int ROWS_UNITS = 4;         // hidden units per workgroup: one per wave
constexpr int ROWS_HBUF = 4;          // offset (floats) of h in the scratch block, behind the arrival counter

__host__ __device__ constexpr int rows_lds_floats(int MT, int K, int H) {
    return MT * (((K + 3) & ~3) > H ? ((K + 3) & ~3) : H) + 4;
}

template <int MT>
__global__ __launch_bounds__(256) void enc_mlp2_rows_kernel(const float *__restrict__ X, int64_t ldx,
                                                            const float *__restrict__ W0, const float *__restrict__ b0,
                                                            const float *__restrict__ W1, const float *__restrict__ b1,
                                                            int M, int K, int H, int N, int act2, float *__restrict__ Y,
                                                            int64_t ldy, unsigned *counter, float *hbuf, int S) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Kp = (K + 3) & ~3;
    int *last = reinterpret_cast<int *>(lds + MT * (Kp > H ? Kp : H));

    // ---- the rows of X, zero-padded to MT x Kp (any ldx, any alignment)
    for (int i = tid; i < MT * Kp; i += 256) {
        const int m = i / Kp, k = i - m * Kp;
        const bool ok = m < M && k < K;
        const float v = X[ok ? (int64_t)m * ldx + k : 0];
        lds[i] = ok ? v : 0.0f;
    }
    __syncthreads();

    // ---- layer 1: hidden unit j of every row (grid = H / 4: j < H)
    {
        const int j = blockIdx.x * ROWS_UNITS + wave;
        const float *wrow = W0 + (int64_t)j * K;
        const bool vec = ((uintptr_t)wrow & 15) == 0;
        float acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = 0.0f;
        for (int k = 4 * lane; k < K; k += 256) {
            float w[4];
            if (vec && k + 3 < K) {
                const float4 t = *reinterpret_cast<const float4 *>(wrow + k);
                w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = wrow[k + i < K ? k + i : 0];
                    w[i] = k + i < K ? v : 0.0f;
                }
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float4 x = *reinterpret_cast<const float4 *>(lds + m * Kp + k);
                acc[m] = fmaf(w[0], x.x, acc[m]);
                acc[m] = fmaf(w[1], x.y, acc[m]);
                acc[m] = fmaf(w[2], x.z, acc[m]);
                acc[m] = fmaf(w[3], x.w, acc[m]);
            }
        }
        float mine = 0.0f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc[m] += __shfl_xor(acc[m], off);
            if (lane == m) mine = acc[m];
        }
        if (lane < M) hbuf[lane * H + j] = fmaxf(mine + b0[j], 0.0f);
    }

    // ---- arrival: the last workgroup goes on, every other one ends here
    __threadfence();
    __syncthreads();   // (also: every read of the X image is behind us)
    if (tid == 0) *last = atomicAdd(counter, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!*last) return;
    __threadfence();
    if (tid == 0) atomicExch(counter, 0u);
    for (int i = tid; i < MT * H; i += 256)
        lds[i] = i < M * H ? __hip_atomic_load(hbuf + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    __syncthreads();

    // ---- layer 2: S lanes per output column, 256 / S columns per pass (the pass count is uniform: the shuffles are too)
    const int g = tid / S, s = tid - g * S, chunks = H >> 2;
    const bool vec1 = ((uintptr_t)W1 & 15) == 0;   // (rows of H floats, H % 32 == 0: all rows aligned alike)
    for (int n0 = 0; n0 < N; n0 += 256 / S) {
        const int n = n0 + g;
        const float *wrow = W1 + (int64_t)(n < N ? n : N - 1) * H;
        float acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = 0.0f;
        for (int c = s; c < chunks; c += S) {
            float w[4];
            if (vec1) {
                const float4 t = *reinterpret_cast<const float4 *>(wrow + 4 * c);
                w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = wrow[4 * c + i];
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float4 x = *reinterpret_cast<const float4 *>(lds + m * H + 4 * c);
                acc[m] = fmaf(w[0], x.x, acc[m]);
                acc[m] = fmaf(w[1], x.y, acc[m]);
                acc[m] = fmaf(w[2], x.z, acc[m]);
                acc[m] = fmaf(w[3], x.w, acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
            for (int off = S >> 1; off > 0; off >>= 1) acc[m] += __shfl_xor(acc[m], off);
        if (s == 0 && n < N) {
            const float bias = b1[n];
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < M) Y[(int64_t)m * ldy + n] = act_fwd(acc[m] + bias, act2);
        }
    }
}

bool rows_covered(int M, int K, int H, int N) {
    return M >= 1 && M <= ROWS_MAX_M && K >= 1 && K <= ROWS_MAX_K && N >= 1 && N <= ROWS_MAX_N && H >= 32 && H <= MAX_H &&
           (H & 31) == 0;
}

// lanes per output column of layer 2: the largest power of two that keeps one pass (N S <= 256), within 8 .. 64 (8 lanes
// read one 128-byte line of a W1 row together)
int rows_split(int N) {
    int S = 64;
    while (S > 8 && N * S > 256) S >>= 1;
    return S;
}

// where the few-row forward measured faster than the launches a plan records otherwise (profiles/mlp_encoder.md, "Acting")
// Measured at 1 and 4 rows (us per call, few-row against what the plan records otherwise):
//   17 -> 128 -> 17     7.76 / 10.12 against the fused tile launch's 6.54 / 7.00: slower, stays off (as all K <= 32)
//   324 -> 256 -> 2     9.62 / 13.61 against the per-layer launches' 23.80 / 24.05: faster at both
//   376 -> 128 -> 376   18.29 against 19.19 at 1 row: faster (by more than the spread); 36.04 against 19.77 at 4: slower
// The region is those points and what does no more work than one of them: K inside the measured 324 .. 376 only;
// up to 4 rows with N <= 4 (the 64-lanes-per-column split measured at N 2, any covered H: 256 was measured); one row
// with H <= 128 and N <= 376.  5 .. 16 rows were not measured and stay off.
bool rows_measured_faster(int M, int K, int H, int N) {
    if (K < 324 || K > 376) return false;
    if (M <= 4 && N <= 4) return true;
    return M == 1 && H <= 128 && N <= 376;
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

extern "C" int ssac_enc_mlp2_rows_covered(int M, int K, int H, int N) { return rows_covered(M, K, H, N) ? 1 : 0; }

extern "C" int ssac_enc_mlp2_rows_supported(int M, int K, int H, int N) {
    // the shapes the few-row forward is the default for: those it MEASURED faster at than what an acting plan records
    // otherwise (profiles/mlp_encoder.md, "Acting").  K ranges that were not measured stay off.
    return rows_covered(M, K, H, N) && rows_measured_faster(M, K, H, N) ? 1 : 0;
}

extern "C" int ssac_enc_mlp2_fwd_rows(const float *X, int64_t ldx, const float *W0, const float *b0, const float *W1,
                                      const float *b1, int M, int K, int H, int N, int act2, float *Y, int64_t ldy,
                                      float *scratch, void *stream) {
    if (!rows_covered(M, K, H, N))
        return ssac_fail("ssac_enc_mlp2_fwd_rows: shape not covered (see ssac_enc_mlp2_rows_covered)");
    if (ldx < K || ldy < N || act2 < ACT_NONE || act2 > ACT_TANH)
        return ssac_fail("ssac_enc_mlp2_fwd_rows: bad stride or activation");
    if (!scratch || ((uintptr_t)scratch & 3)) return ssac_fail("ssac_enc_mlp2_fwd_rows: scratch must be a float block");
    unsigned *counter = reinterpret_cast<unsigned *>(scratch);
    float *hbuf = scratch + ROWS_HBUF;
    const dim3 grid(H / ROWS_UNITS), block(256);
    const int S = rows_split(N);
    hipStream_t st = (hipStream_t)stream;
    if (M == 1)
        SSAC_LAUNCH(enc_mlp2_rows_kernel<1>, grid, block, (size_t)rows_lds_floats(1, K, H) * sizeof(float), st, X, ldx, W0, b0,
                    W1, b1, M, K, H, N, act2, Y, ldy, counter, hbuf, S);
    else if (M <= 4)
        SSAC_LAUNCH(enc_mlp2_rows_kernel<4>, grid, block, (size_t)rows_lds_floats(4, K, H) * sizeof(float), st, X, ldx, W0, b0,
                    W1, b1, M, K, H, N, act2, Y, ldy, counter, hbuf, S);
    else
        SSAC_LAUNCH(enc_mlp2_rows_kernel<16>, grid, block, (size_t)rows_lds_floats(16, K, H) * sizeof(float), st, X, ldx, W0,
                    b0, W1, b1, M, K, H, N, act2, Y, ldy, counter, hbuf, S);
    return ssac_check_launch("enc_mlp2_fwd_rows");
}

extern "C" int ssac_enc_mlp2_bwd(const float *dY, int64_t ldd, const float *Y, int64_t ldy, const float *H_save,
                                 const float *W1, int M, int H, int N, int act2, float *dZ1, float *dZ0, void *stream) {
    if (!covered(M, 1, H, N)) return ssac_fail("ssac_enc_mlp2_bwd: shape not covered (see ssac_enc_mlp2_covered)");
    if (ldd < N || ldy < N || act2 < ACT_NONE || act2 > ACT_TANH) return ssac_fail("ssac_enc_mlp2_bwd: bad stride or activation");
    SSAC_LAUNCH(enc_mlp2_bwd_kernel, dim3((M + ROWS - 1) / ROWS), dim3(256), (size_t)bwd_lds_floats(H) * sizeof(float),
                (hipStream_t)stream, dY, ldd, Y, ldy, H_save, W1, M, H, N, act2, dZ1, dZ0);
    return ssac_check_launch("enc_mlp2_bwd");
}
