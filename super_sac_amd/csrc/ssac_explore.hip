// "Head, then exploration process" of the TD target's next action in ONE launch (learning_utils.py:329-338 on
// :48-59): what ssac_tanh_normal_fwd + ssac_exploration_noise, or ssac_det_action_fwd with noise, do in two kernels
// and with a by-value scale.  The launch exists so that a critic update that carries an exploration process can be
// RECORDED: the scale is read from a device-visible float (the aux word of this update's slot of the input ring) and
// both noise fields can come from the engine's Philox stream, so nothing in the argument bytes changes per update.
//
// The arithmetic is that of tanh_normal_fwd_kernel, det_action_fwd_kernel and exploration_noise_kernel
// (ssac_elementwise.hip), expression by expression and in the same order (the library is built with
// -ffp-contract=off): given the same eps, noise and scale the action -- and log pi -- are the same bits.  Byte/row
// work: one thread per (row, action dimension), consecutive threads walk one row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssac_internal.h"
#include "ssac_philox.h"

namespace {

constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;
constexpr float LOG_2 = 0.69314718055994530942f;
// the process noise has its own Philox key (seed ^ salt): it shares the update's draw number with the head's eps and
// is still independent of it
constexpr uint64_t EXPLORE_KEY_SALT = 0xE5A1C0DE0D15EA5EULL;
// one workgroup holds WHOLE rows (the tanh-normal head sums a row's log-density terms in index order): act_dim <= 256
constexpr int EXPLORE_THREADS = 256;

__device__ __forceinline__ float softplus_f(float x) {
    // F.softplus, beta=1, threshold=20
    return x > 20.0f ? x : log1pf(expf(x));
}

struct ExploreArgs {
    const float *out; int64_t ld_out;   // the actor's head output: n_rows x 2A (tanh-normal) or n_rows x A (deterministic)
    const float *eps;                   // (n_rows x A) head noise, or null: Philox under `seed`
    const float *noise;                 // (n_rows x A) process noise, or null: Philox under seed ^ EXPLORE_KEY_SALT
    RngArgs rng;
    const float *scale_ptr;             // the process's current scale in device-visible memory, or null: `scale`
    float scale, clip, lo, hi;
    int n_rows, A, rows_per_wg;
    float *act; int64_t ld_act, col0;
    float *logp;                        // (n_rows) log pi of the tanh-normal sample BEFORE the process, or null
};

template <bool TANH_NORMAL>
__global__ __launch_bounds__(EXPLORE_THREADS) void explore_action_kernel(ExploreArgs p) {
    __shared__ float terms[EXPLORE_THREADS];
    const int A = p.A;
    const int r = threadIdx.x / A, i = threadIdx.x - r * A;
    const int b = blockIdx.x * p.rows_per_wg + r;
    const bool live = r < p.rows_per_wg && b < p.n_rows;
    if (live) {
        const bool philox = !p.noise || (TANH_NORMAL && !p.eps);
        const int64_t draw = philox ? rng_draw(p.rng) : 0;   // offset + *counter, as ssac_rng documents
        float a;
        if (TANH_NORMAL) {
            const float mu = p.out[b * p.ld_out + i];
            const float raw = p.out[b * p.ld_out + A + i];
            const float log_std = p.lo + 0.5f * (p.hi - p.lo) * (tanhf(raw) + 1.0f);
            const float sd = expf(log_std);
            const float e = p.eps ? p.eps[(int64_t)b * A + i] : philox_normal(p.rng.seed, draw, b, i);
            const float u = mu + sd * e;
            a = tanhf(u);
            if (p.logp) {
                const float dlt = u - mu;
                const float base = -(dlt * dlt) / (2.0f * sd * sd) - logf(sd) - LOG_SQRT_2PI;
                const float ladj = 2.0f * (LOG_2 - u - softplus_f(-2.0f * u));
                terms[threadIdx.x] = base - ladj;
            }
        } else {
            a = tanhf(p.out[b * p.ld_out + i]);
        }
        const float scale = p.scale_ptr ? *p.scale_ptr : p.scale;
        const float n = p.noise ? p.noise[(int64_t)b * A + i] : philox_normal(p.rng.seed ^ EXPLORE_KEY_SALT, draw, b, i);
        float nz = scale * n;
        if (p.clip > 0.0f) nz = fminf(fmaxf(nz, -p.clip), p.clip);
        p.act[b * p.ld_act + p.col0 + i] = fminf(fmaxf(a + nz, -1.0f + 1e-6f), 1.0f - 1e-6f);
    }
    if (TANH_NORMAL && p.logp) {
        __syncthreads();
        if (live && i == 0) {
            // tanh_normal_fwd_kernel's summation: lp = 0, then += term in index order
            float lp = 0.0f;
            for (int k = 0; k < A; ++k) lp += terms[threadIdx.x + k];
            p.logp[b] = lp;
        }
    }
}

}  // namespace

extern "C" int ssac_explore_action(const float *out, int64_t ld_out, int tanh_normal, float log_std_lo,
                                   float log_std_hi, const float *eps, const float *noise, const ssac_rng *rng,
                                   const float *scale_ptr, float scale, float noise_clip, int n_rows, int act_dim,
                                   float *act_dst, int64_t ld_act, int64_t act_col0, float *logp, void *stream) {
    if (!out || !act_dst) return ssac_fail("ssac_explore_action: null argument");
    if (act_dim <= 0 || act_dim > EXPLORE_THREADS) return ssac_fail("ssac_explore_action: act_dim must be in [1, 256]");
    if (ld_out < (tanh_normal ? 2 : 1) * (int64_t)act_dim || act_col0 < 0 || ld_act < act_col0 + act_dim)
        return ssac_fail("ssac_explore_action: row strides do not cover the head output / the action columns");
    if (!tanh_normal && (eps || logp)) return ssac_fail("ssac_explore_action: the deterministic head takes no eps and has no log pi");
    if (!rng && (!noise || (tanh_normal && !eps)))
        return ssac_fail("ssac_explore_action: a noise field without a buffer needs the Philox stream (rng)");
    if (n_rows <= 0) return 0;
    ExploreArgs p;
    p.out = out; p.ld_out = ld_out; p.eps = eps; p.noise = noise;
    p.rng = rng ? RngArgs{rng->seed, rng->counter, rng->offset} : RngArgs{0, nullptr, 0};
    p.scale_ptr = scale_ptr; p.scale = scale; p.clip = noise_clip; p.lo = log_std_lo; p.hi = log_std_hi;
    p.n_rows = n_rows; p.A = act_dim; p.rows_per_wg = EXPLORE_THREADS / act_dim;
    p.act = act_dst; p.ld_act = ld_act; p.col0 = act_col0; p.logp = logp;
    const dim3 grid((n_rows + p.rows_per_wg - 1) / p.rows_per_wg), block(EXPLORE_THREADS);
    if (tanh_normal)
        SSAC_LAUNCH(explore_action_kernel<true>, grid, block, 0, (hipStream_t)stream, p);
    else
        SSAC_LAUNCH(explore_action_kernel<false>, grid, block, 0, (hipStream_t)stream, p);
    return ssac_check_launch("explore_action");
}
