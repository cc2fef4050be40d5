// Ensemble-member pieces of a recorded critic update with ensemble_size > 1 (SUNRISE) on gfx950:
//   ssac_members_sunrise_weights   the backup weights of ALL E member batches from one packed target-critic forward
//   ssac_group_norms_pick          ssac_group_norms over the sum-of-squares buffer a device-resident int32 selects
//
// Both are small VALU kernels (a few KB of input): one thread per (member batch, row), wave64 shuffles + an LDS tree for
// the batch statistics.  Their fp32 expressions and summation orders are those of ensemble_min_select_kernel ->
// sunrise_weights_kernel and of group_norms_kernel (ssac_elementwise.hip), operation by operation, so a recorded update
// and the per-member launches of an eager one leave the same bits (tests/test_hip_members_kernels.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssac_internal.h"

namespace {

constexpr int RED_THREADS = 1024;   // (as the single-workgroup reductions of ssac_elementwise.hip: the order is part of the result)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide reductions for <= 1024 threads; `scratch` is 16 floats of LDS; result broadcast (ssac_elementwise.hip's)
template <int OP>  // 0 sum, 1 max, 2 min
__device__ float block_reduce(float v, float *scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = OP == 0 ? wave_sum(v) : (OP == 1 ? wave_max(v) : wave_min(v));
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float r = scratch[0];
    for (int w = 1; w < nw; ++w) r = OP == 0 ? r + scratch[w] : (OP == 1 ? fmaxf(r, scratch[w]) : fminf(r, scratch[w]));
    return r;
}

// Workgroup i = member batch i (rows [i B, (i + 1) B) of the stacked batch).  q: (E N nets, E B rows, q_dim), net k N + j =
// net j of member k's target critics.  Per row: Qbar_k = min_j q[k N + j][row][sel] (sel = the taken action's column for
// discrete critics), w = sigmoid(-std_k(Qbar_k) temp) + 0.5.  The LAST workgroup also leaves mean / max / min / std of its
// batch's weights in logs[0..3]: the reference's member loop overwrites them and the last member's stand.
__global__ __launch_bounds__(RED_THREADS) void members_sunrise_weights_kernel(
        const float *__restrict__ q, int E, int N, int B, int q_dim, float temp, const float *__restrict__ act,
        int64_t ld_act, float *__restrict__ w, float *__restrict__ logs) {
    __shared__ float scratch[16];
    const int i = blockIdx.x;
    const int64_t rows = (int64_t)E * B;
    float *wi = w + (int64_t)i * B;
    float s = 0.f, mx = -INFINITY, mn = INFINITY;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const int64_t row = (int64_t)i * B + b;
        int sel = 0;
        if (q_dim > 1) {
            sel = (int)act[row * ld_act];
            sel = sel < 0 ? 0 : (sel >= q_dim ? q_dim - 1 : sel);   // (a valid action index always is: never read outside q)
        }
        const int64_t e = row * q_dim + sel;
        float qk[SSAC_MAX_MEMBERS];
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < SSAC_MAX_MEMBERS; ++k) {
            if (k < E) {
                float v = q[(int64_t)(k * N) * rows * q_dim + e];
                for (int j = 1; j < N; ++j) v = fminf(v, q[(int64_t)(k * N + j) * rows * q_dim + e]);
                qk[k] = v;
                m += v;
            }
        }
        m /= (float)E;
        float var = 0.f;
#pragma unroll
        for (int k = 0; k < SSAC_MAX_MEMBERS; ++k) {
            if (k < E) {
                const float d = qk[k] - m;
                var += d * d;
            }
        }
        const float sd = sqrtf(var / (float)(E - 1));
        const float wv = 1.0f / (1.0f + expf(sd * temp)) + 0.5f;  // sigmoid(-sd*temp) + 0.5
        wi[b] = wv;
        s += wv;
        mx = fmaxf(mx, wv);
        mn = fminf(mn, wv);
    }
    if (i != E - 1 || !logs) return;   // (uniform over the workgroup)
    const float mean = block_reduce<0>(s, scratch) / (float)B;
    mx = block_reduce<1>(mx, scratch);
    mn = block_reduce<2>(mn, scratch);
    float sv = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float d = wi[b] - mean;   // (this thread's own store above)
        sv += d * d;
    }
    const float var = block_reduce<0>(sv, scratch) / (float)(B > 1 ? B - 1 : 1);
    if (threadIdx.x == 0) {
        logs[0] = mean; logs[1] = mx; logs[2] = mn; logs[3] = sqrtf(var);
    }
}

struct PickTable {
    const float *buf[SSAC_MAX_MEMBERS];
    int count;
};

// group_norms_kernel over table.buf[*pick]: the recorded argument bytes hold every member's buffer, the update's slot
// says which one is read
__global__ void group_norms_pick_kernel(PickTable table, const int32_t *__restrict__ pick, int group_size,
                                        const ssac_adam_ctl *scale, float *out) {
    __shared__ float scratch[16];
    int p = *pick;
    p = p < 0 ? 0 : (p >= table.count ? table.count - 1 : p);   // (never outside the table, whatever the word holds)
    const float *sumsq = table.buf[0];
#pragma unroll
    for (int k = 1; k < SSAC_MAX_MEMBERS; ++k)
        if (k == p) sumsq = table.buf[k];   // (a select chain: no dynamically indexed kernel-argument array)
    float s = 0.f;
    for (int i = threadIdx.x; i < group_size; i += blockDim.x) s += sumsq[(int64_t)blockIdx.x * group_size + i];
    const float tot = block_reduce<0>(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrtf(tot) * (scale ? scale->clip_coef : 1.0f);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int ssac_members_sunrise_weights(const float *q, int n_members, int n_nets, int n_rows, int q_dim, float temp,
                                            const float *act, int64_t ld_act, float *w, float *logs, void *stream) {
    if (!q || !w || n_members < 2 || n_members > SSAC_MAX_MEMBERS || n_nets < 1 || n_rows < 1 || q_dim < 1)
        return ssac_fail("ssac_members_sunrise_weights: bad sizes");
    if (q_dim > 1 && (!act || ld_act < 1))
        return ssac_fail("ssac_members_sunrise_weights: q_dim > 1 needs the taken actions");
    SSAC_LAUNCH(members_sunrise_weights_kernel, dim3(n_members), dim3(RED_THREADS), 0, ST, q, n_members, n_nets, n_rows,
                q_dim, temp, act, ld_act, w, logs);
    return ssac_check_launch("members_sunrise_weights");
}

extern "C" int ssac_group_norms_pick(const float *const *sumsq, int n_buffers, const int32_t *pick, int n_groups,
                                     int group_size, const ssac_adam_ctl *scale_by_clip, float *out, void *stream) {
    if (!sumsq || !pick || !out || n_buffers < 1 || n_buffers > SSAC_MAX_MEMBERS)
        return ssac_fail("ssac_group_norms_pick: bad arguments");
    if (n_groups <= 0 || group_size <= 0) return 0;
    PickTable t{};
    for (int k = 0; k < SSAC_MAX_MEMBERS; ++k) {
        if (k < n_buffers && !sumsq[k]) return ssac_fail("ssac_group_norms_pick: null buffer");
        t.buf[k] = sumsq[k < n_buffers ? k : 0];
    }
    t.count = n_buffers;
    SSAC_LAUNCH(group_norms_pick_kernel, dim3(n_groups), dim3(64), 0, ST, t, pick, group_size, scale_by_clip, out);
    return ssac_check_launch("group_norms_pick");
}
