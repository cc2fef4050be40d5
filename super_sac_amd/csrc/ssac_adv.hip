// The stacked batch of the advantage estimator (adv_estimator.py:58-79) in ONE launch: block 0 = (s, a_data), blocks
// 1..n = (s, a_k) with a_k a sample of the member's policy -- what two torch copy kernels plus one
// ssac_tanh_normal_fwd / ssac_det_action_fwd launch per sample (and, for the tanh-normal head, one torch.randn per
// sample) do today.  The launch exists so that a critic update that refreshes the replay priorities (AWAC / AFBC:
// update_priorities=True) can be RECORDED: a launch list holds no torch kernel, and the candidates' noise can come
// from the engine's Philox stream, so nothing in the argument bytes changes per update.
//
// The candidate arithmetic is that of tanh_normal_fwd_kernel / det_action_fwd_kernel (ssac_elementwise.hip),
// expression by expression and in the same order (the library is built with -ffp-contract=off): given the same eps the
// action columns are the same bits.  Memory-bound and tiny ((1 + n) * n_rows * (S + A) floats written): one thread
// per unit of a row, consecutive threads walk one output row, so the stores of a wave are contiguous.  A unit is four
// state floats (one 16-byte load and store) where ld_s, S, S + A and both base addresses are multiples of four floats,
// else one float; the action columns are always one float per thread.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssac_internal.h"
#include "ssac_philox.h"

namespace {

// the candidates' noise has its own Philox key (seed ^ salt): it shares the update's draw number with the TD target's
// head noise (key seed) and process noise (key seed ^ 0xE5A1C0DE0D15EA5E) and is still independent of both
constexpr uint64_t ADV_KEY_SALT = 0xADC0FFEE5A3B1E57ULL;
constexpr int ADV_THREADS = 256;
constexpr int ADV_MAX_ACT = 256;   // ssac_explore_action's limit

struct AdvArgs {
    const float *s; int64_t ld_s;       // n_rows x S state rows
    const float *act; int64_t ld_act;   // n_rows x A data actions
    const float *out; int64_t ld_out;   // the actor's head output: n_rows x 2A (tanh-normal) or n_rows x A (deterministic)
    const float *eps;                   // (n_samples * n_rows x A), sample-major, or null: Philox under seed ^ ADV_KEY_SALT
    RngArgs rng;
    float lo, hi;
    int n_rows, S, A, n_samples;
    float *X;                           // (1 + n_samples) * n_rows x (S + A), dense
};

template <bool TANH_NORMAL, int VEC>
__global__ __launch_bounds__(ADV_THREADS) void adv_candidates_kernel(AdvArgs p) {
    const int S = p.S, A = p.A, W = S + A;
    const int s_units = S / VEC, units = s_units + A;   // units of one output row
    const int64_t total = (int64_t)(1 + p.n_samples) * p.n_rows * units;
    const int64_t t = blockIdx.x * (int64_t)ADV_THREADS + threadIdx.x;
    if (t >= total) return;
    const int64_t r = t / units;          // output row: k * n_rows + b
    const int u = (int)(t - r * units);
    const int k = (int)(r / p.n_rows), b = (int)(r - (int64_t)k * p.n_rows);
    float *dst = p.X + r * W;
    if (u < s_units) {
        const float *src = p.s + b * p.ld_s;
        if (VEC == 4)
            reinterpret_cast<float4 *>(dst)[u] = reinterpret_cast<const float4 *>(src)[u];
        else
            dst[u] = src[u];
        return;
    }
    const int i = u - s_units;
    float a;
    if (k == 0) {
        a = p.act[b * p.ld_act + i];
    } else if (TANH_NORMAL) {
        const float mu = p.out[b * p.ld_out + i];
        const float raw = p.out[b * p.ld_out + A + i];
        const float log_std = p.lo + 0.5f * (p.hi - p.lo) * (tanhf(raw) + 1.0f);
        const float sd = expf(log_std);
        const int64_t row = (int64_t)(k - 1) * p.n_rows + b;   // row of the (n_samples * n_rows x A) noise field
        const float e = p.eps ? p.eps[row * A + i] : philox_normal(p.rng.seed ^ ADV_KEY_SALT, rng_draw(p.rng), (int)row, i);
        const float v = mu + sd * e;
        a = tanhf(v);
    } else {
        a = tanhf(p.out[b * p.ld_out + i]);
    }
    dst[S + i] = a;
}

}  // namespace

extern "C" int ssac_adv_candidates(const float *s, int64_t ld_s, const float *act, int64_t ld_act, const float *out,
                                   int64_t ld_out, int tanh_normal, float log_std_lo, float log_std_hi, const float *eps,
                                   const ssac_rng *rng, int n_rows, int state_dim, int act_dim, int n_samples, float *X,
                                   void *stream) {
    if (!s || !act || !out || !X) return ssac_fail("ssac_adv_candidates: null argument");
    if (act_dim <= 0 || act_dim > ADV_MAX_ACT) return ssac_fail("ssac_adv_candidates: act_dim must be in [1, 256]");
    if (state_dim <= 0 || n_samples <= 0) return ssac_fail("ssac_adv_candidates: state_dim and n_samples must be positive");
    if (ld_s < state_dim || ld_act < act_dim || ld_out < (tanh_normal ? 2 : 1) * (int64_t)act_dim)
        return ssac_fail("ssac_adv_candidates: row strides do not cover the state / the action / the head output");
    if (!tanh_normal && eps) return ssac_fail("ssac_adv_candidates: the deterministic head takes no eps");
    if (tanh_normal && !eps && !rng)
        return ssac_fail("ssac_adv_candidates: noise without a buffer needs the Philox stream (rng)");
    if (n_rows <= 0) return 0;
    if ((int64_t)n_samples * n_rows > INT32_MAX) return ssac_fail("ssac_adv_candidates: n_samples * n_rows exceeds the noise field's row range");
    AdvArgs p;
    p.s = s; p.ld_s = ld_s; p.act = act; p.ld_act = ld_act; p.out = out; p.ld_out = ld_out; p.eps = eps;
    p.rng = rng ? RngArgs{rng->seed, rng->counter, rng->offset} : RngArgs{0, nullptr, 0};
    p.lo = log_std_lo; p.hi = log_std_hi;
    p.n_rows = n_rows; p.S = state_dim; p.A = act_dim; p.n_samples = n_samples; p.X = X;
    // 16-byte state units need every row of s and of X to start on a 16-byte boundary and S to be whole units
    const bool vec = state_dim % 4 == 0 && ld_s % 4 == 0 && (state_dim + act_dim) % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(s) & 15) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    const int units = (vec ? state_dim / 4 : state_dim) + act_dim;
    const int64_t total = (int64_t)(1 + n_samples) * n_rows * units;
    const int64_t blocks = (total + ADV_THREADS - 1) / ADV_THREADS;
    if (blocks > INT32_MAX) return ssac_fail("ssac_adv_candidates: batch too large for one launch");
    const dim3 grid((unsigned)blocks), block(ADV_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (tanh_normal && vec) SSAC_LAUNCH((adv_candidates_kernel<true, 4>), grid, block, 0, st, p);
    else if (tanh_normal) SSAC_LAUNCH((adv_candidates_kernel<true, 1>), grid, block, 0, st, p);
    else if (vec) SSAC_LAUNCH((adv_candidates_kernel<false, 4>), grid, block, 0, st, p);
    else SSAC_LAUNCH((adv_candidates_kernel<false, 1>), grid, block, 0, st, p);
    return ssac_check_launch("adv_candidates");
}
