// Beta policy head (reference nets/distributions.py:18-53, BetaDist over torch.distributions.Beta) on gfx950:
// sampler, log-density, mean, and the backward pass through torch's Dirichlet reparameterisation gradient.
//
// Per action element (b, i) of the head output vec (n_rows x 2A):
//   alpha = 1 + softplus(vec[b][i]), beta = 1 + softplus(vec[b][A + i])     (F.softplus, threshold 20; fp32)
//   x ~ Beta(alpha, beta), a = 2x - 1                                        (fp32)
//   log pi_b = sum_i xlogy(alpha-1, x) + xlogy(beta-1, 1-x) + lgamma(alpha+beta) - lgamma(alpha) - lgamma(beta) - log 2
// The special functions (lgamma, digamma, the port of ATen's dirichlet_grad_one) run in fp64, as torch's CPU kernels
// evaluate them; alpha, beta, 1 - x and the action stay in fp32 where torch computes them in fp32.
//
// One thread per element.  These are a few thousand elements per update, latency-bound: no MFMA, no LDS beyond the
// per-row log-density sum, which is done in a fixed order by the row's first lane (no atomics: a replay is bit-identical).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ssac_internal.h"
#include "ssac_philox.h"

namespace {

constexpr int BETA_THREADS = 256;
constexpr int BETA_MAX_ATTEMPTS = 32;                      // Marsaglia-Tsang rejection rounds per Gamma draw
constexpr uint64_t BETA_KEY_SALT = 0x5A17BE7A5A17BE7AULL;   // Beta draws use their own Philox key (seed ^ salt)
constexpr double LOG_2_D = 0.69314718055994530942;
constexpr double PI_D = 3.14159265358979323846;

// ATen/native/Distributions.h: digamma_one (Cephes), asymptotic coefficients
__constant__ double PSI_A[7] = {
    8.33333333333333333333E-2, -2.10927960927960927961E-2, 7.57575757575757575758E-3, -4.16666666666666666667E-3,
    3.96825396825396825397E-3, -8.33333333333333333333E-3, 8.33333333333333333333E-2,
};

// ATen/native/Distributions.h: dirichlet_grad_one, rational correction coefficients
__constant__ double DIR_C[2][3][3][4] = {
    {{{1.003668233, -0.01061107488, -0.0657888334, 0.01201642863},
      {0.6336835991, -0.3557432599, 0.05486251648, -0.001465281033},
      {-0.03276231906, 0.004474107445, 0.002429354597, -0.0001557569013}},
     {{0.221950385, -0.3187676331, 0.01799915743, 0.01074823814},
      {-0.2951249643, 0.06219954479, 0.01535556598, 0.001550077057},
      {0.02155310298, 0.004170831599, 0.001292462449, 6.976601077e-05}},
     {{-0.05980841433, 0.008441916499, 0.01085618172, 0.002319392565},
      {0.02911413504, 0.01400243777, -0.002721828457, 0.000751041181},
      {0.005900514878, -0.001936558688, -9.495446725e-06, 5.385558597e-05}}},
    {{{1, -0.02924021934, -0.04438342661, 0.007285809825},
      {0.6357567472, -0.3473456711, 0.05454656494, -0.002407477521},
      {-0.03301322327, 0.004845219414, 0.00231480583, -0.0002307248149}},
     {{0.5925320577, -0.1757678135, 0.01505928619, 0.000564515273},
      {0.1014815858, -0.06589186703, 0.01272886114, -0.0007316646956},
      {-0.007258481865, 0.001096195486, 0.0003934994223, -4.12701925e-05}},
     {{0.06469649321, -0.0236701437, 0.002902096474, -5.896963079e-05},
      {0.001925008108, -0.002869809258, 0.0008000589141, -6.063713228e-05},
      {-0.0003477407336, 6.959756487e-05, 1.097287507e-05, -1.650964693e-06}}},
};

__device__ __forceinline__ float softplus20(float v) { return v > 20.0f ? v : log1pf(expf(v)); }

// torch's softplus backward (threshold 20), fp32
__device__ __forceinline__ float softplus20_bwd(float v, float g) {
    if (v > 20.0f) return g;
    const float z = expf(v);
    return g * z / (z + 1.0f);
}

__device__ double digamma_d(double x) {
    const double PSI_10 = 2.25175258906672110764;
    if (x == 0) return INFINITY;
    double additional = 0;
    const bool is_int = x == floor(x);
    if (x < 0) {
        if (is_int) return INFINITY;
        additional = -PI_D / tan(PI_D * x);
        x = 1 - x;
    }
    double result = 0;
    while (x < 10) {
        result -= 1 / x;
        x += 1;
    }
    if (x == 10) return result + PSI_10 + additional;
    double y = 0;
    if (x < 1.0e17) {
        const double z = 1.0 / (x * x);
        double p = 0;
        for (int k = 0; k <= 6; ++k) p = p * z + PSI_A[k];
        y = z * p;
    }
    return result + log(x) - (0.5 / x) - y + additional;
}

// ---- port of ATen's dirichlet_grad_one<double, double> (torch._dirichlet_grad): the scaled reparameterised gradient
//      -(d/d alpha cdf(x; alpha, beta)) / pdf(x; alpha, beta) / (1 - x) of a Beta(alpha, total - alpha) draw x
__device__ double beta_grad_alpha_small(double x, double alpha, double beta) {
    const double factor = digamma_d(alpha) - digamma_d(alpha + beta) - log(x);
    double numer = 1;
    double series = numer / alpha * (factor + 1 / alpha);
    for (int i = 1; i <= 10; ++i) {
        const double ci = (double)i;
        numer *= (ci - beta) * x / ci;
        const double denom = alpha + ci;
        series += numer / denom * (factor + 1 / denom);
    }
    const double result = x * pow(1 - x, -beta) * series;
    return isnan(result) ? 0.0 : result;
}

__device__ double beta_grad_beta_small(double x, double alpha, double beta) {
    const double factor = digamma_d(alpha + beta) - digamma_d(beta);
    double numer = 1, betas = 1, dbetas = 0, series = factor / alpha;
    for (int i = 1; i <= 8; ++i) {
        const double ci = (double)i;
        numer *= -x / ci;
        dbetas = dbetas * (beta - ci) + betas;
        betas = betas * (beta - ci);
        series += numer / (alpha + ci) * (dbetas + factor * betas);
    }
    const double result = -pow(1 - x, 1 - beta) * series;
    return isnan(result) ? 0.0 : result;
}

__device__ double beta_grad_alpha_mid(double x, double alpha, double beta) {
    const double total = alpha + beta;
    const double mean = alpha / total;
    const double std = sqrt(alpha * beta / (total + 1)) / total;
    if (mean - 0.1 * std <= x && x <= mean + 0.1 * std) {
        const double poly = 47 * x * (beta * beta) * (beta * beta) + alpha * (
                            (43 + 20 * (16 + 27 * beta) * x) * (beta * beta) * beta + alpha * (
                            3 * (59 + 180 * beta - 90 * x) * (beta * beta) + alpha * (
                            (453 + 1620 * beta * (1 - x) - 455 * x) * beta + alpha * (
                            8 * (1 - x) * (135 * beta - 11)))));
        const double prefactor_num = (1 + 12 * alpha) * (1 + 12 * beta) / (total * total);
        const double prefactor_den = 12960 * alpha * alpha * alpha * beta * beta * (1 + 12 * total);
        return prefactor_num / (1 - x) * poly / prefactor_den;
    }
    const double prefactor = -x / sqrt(2 * alpha * beta / total);
    const double stirling = (1 + 1 / (12 * alpha) + 1 / (288 * alpha * alpha)) *
                            (1 + 1 / (12 * beta) + 1 / (288 * beta * beta)) /
                            (1 + 1 / (12 * total) + 1 / (288 * total * total));
    const double term1_num = 2 * (alpha * alpha) * (x - 1) + alpha * beta * (x - 1) - x * (beta * beta);
    const double axbx = alpha * (x - 1) + beta * x;
    const double term1_den = sqrt(2 * alpha / beta) * pow(total, 1.5) * axbx * axbx;
    const double term1 = term1_num / term1_den;
    const double term2 = 0.5 * log(alpha / (total * x));
    const double term3_num = sqrt(8 * alpha * beta / total);
    const double term3_den = beta * x + alpha * (x - 1);
    const double term3 = term3_num / term3_den;
    const double term4_base = beta * log(beta / (total * (1 - x))) + alpha * log(alpha / (total * x));
    const double term4 = pow(term4_base, -1.5);
    const double term1234 = term1 + term2 * (term3 + (x < mean ? term4 : -term4));
    return stirling * prefactor * term1234;
}

__device__ double dirichlet_grad_one(double x, double alpha, double total) {
    const double beta = total - alpha;
    const double boundary = total * x * (1 - x);
    if (x <= 0.5 && boundary < 2.5) return beta_grad_alpha_small(x, alpha, beta);
    if (x >= 0.5 && boundary < 0.75) return -beta_grad_beta_small(1 - x, beta, alpha);
    if (alpha > 6 && beta > 6) return beta_grad_alpha_mid(x, alpha, beta);
    const double u = log(x);
    const double a = log(alpha) - u;
    const double b = log(total) - a;
    const double pow_u[3] = {1, u, u * u};
    const double pow_a[3] = {1, a, a * a};
    double p = 0.0, q = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            const double ua = pow_u[i] * pow_a[j];
            p += ua * (DIR_C[0][i][j][0] + b * (DIR_C[0][i][j][1] + b * (DIR_C[0][i][j][2] + b * DIR_C[0][i][j][3])));
            q += ua * (DIR_C[1][i][j][0] + b * (DIR_C[1][i][j][1] + b * (DIR_C[1][i][j][2] + b * DIR_C[1][i][j][3])));
        }
    }
    const double approx = x * (digamma_d(total) - digamma_d(alpha)) / beta;
    return p / q * approx;
}

// ---- Marsaglia-Tsang Gamma(shape, 1) for shape >= 1 (always true here: shape = 1 + softplus(.)).  Attempt t of Gamma
//      `which` (0: alpha, 1: beta) of element (row, col) at draw number `draw` is one Philox4x32-10 block with counter
//      {row, 2 col + which, draw low word, draw high word | t << 16} under key seed ^ BETA_KEY_SALT: two words -> one
//      Box-Muller normal, one word -> the acceptance uniform.  (Valid for draw numbers below 2^48.)  After
//      BETA_MAX_ATTEMPTS rejections (probability below 0.05^32 per draw) the fallback is d = shape - 1/3, the value at
//      the transformed normal's mode.
__device__ double gamma_mt(uint64_t key, int64_t draw, int row, int col, int which, double shape) {
    const double d = shape - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (int t = 0; t < BETA_MAX_ATTEMPTS; ++t) {
        uint32_t w[4] = {(uint32_t)row, 2u * (uint32_t)col + (uint32_t)which, (uint32_t)draw,
                         (uint32_t)((uint64_t)draw >> 32) | ((uint32_t)t << 16)};
        philox4x32_10(w, (uint32_t)key, (uint32_t)(key >> 32));
        const double u1 = ((double)w[0] + 1.0) * 2.3283064365386963e-10;   // (0, 1]
        const double u2 = (double)w[1] * 2.3283064365386963e-10;           // [0, 1)
        const double u = ((double)w[2] + 0.5) * 2.3283064365386963e-10;    // (0, 1)
        const double z = sqrt(-2.0 * log(u1)) * cos(2.0 * PI_D * u2);
        const double s = 1.0 + c * z;
        if (s <= 0.0) continue;
        const double v = s * s * s;
        if (log(u) < 0.5 * z * z + d - d * v + d * log(v)) return d * v;
    }
    return d;
}

// log-density of one element (the Dirichlet log_prob of [x, 1 - x] minus log 2), fp64
__device__ double beta_elem_logp(float x, float al, float be) {
    const float am1 = al - 1.0f, bm1 = be - 1.0f, omx = 1.0f - x;
    double t = 0.0;
    if (am1 != 0.0f) t += (double)am1 * log((double)x);     // xlogy(0, .) = 0
    if (bm1 != 0.0f) t += (double)bm1 * log((double)omx);
    return t + lgamma((double)al + (double)be) - lgamma((double)al) - lgamma((double)be) - LOG_2_D;
}

// mode: SSAC_BETA_SAMPLE / SSAC_BETA_MEAN / SSAC_BETA_GIVEN (include/ssac_hip.h).  Block = rows_per_block rows x A lanes.
__global__ void beta_fwd_kernel(const float *__restrict__ vec, int64_t ld_vec, int n_rows, int A, int rows_per_block,
                                int mode, const float *__restrict__ xin, int64_t ld_xin, RngArgs r,
                                float *__restrict__ act, int64_t ld_act, int64_t col0, float *__restrict__ logp,
                                float *__restrict__ xsave) {
    __shared__ double lp_row[BETA_THREADS];
    const int t = threadIdx.x;
    const int rl = t / A, i = t - rl * A;
    const int b = blockIdx.x * rows_per_block + rl;
    const bool live = rl < rows_per_block && b < n_rows;
    double lp = 0.0;
    if (live) {
        const float va = vec[(int64_t)b * ld_vec + i], vb = vec[(int64_t)b * ld_vec + A + i];
        const float al = 1.0f + softplus20(va), be = 1.0f + softplus20(vb);
        if (mode == SSAC_BETA_MEAN) {
            act[(int64_t)b * ld_act + col0 + i] = 2.0f * (al / (al + be)) - 1.0f;
        } else {
            float x;
            if (mode == SSAC_BETA_GIVEN) {
                x = (fminf(fmaxf(xin[(int64_t)b * ld_xin + i], -0.99f), 0.99f) + 1.0f) / 2.0f;
            } else if (xin) {
                x = xin[(int64_t)b * ld_xin + i];
            } else {
                const uint64_t key = r.seed ^ BETA_KEY_SALT;
                const int64_t draw = rng_draw(r);
                const double g1 = gamma_mt(key, draw, b, i, 0, (double)al);
                const double g2 = gamma_mt(key, draw, b, i, 1, (double)be);
                x = (float)(g1 / (g1 + g2));
                // nudge into the open interval: x in [FLT_MIN, 1 - 2^-24]
                x = fminf(fmaxf(x, FLT_MIN), 0.99999994f);
            }
            if (mode == SSAC_BETA_SAMPLE && act) act[(int64_t)b * ld_act + col0 + i] = 2.0f * x - 1.0f;
            if (xsave) xsave[(int64_t)b * A + i] = x;
            lp = beta_elem_logp(x, al, be);
        }
    }
    if (mode == SSAC_BETA_MEAN || !logp) return;   // (kernel arguments: uniform over the block)
    lp_row[t] = lp;
    __syncthreads();
    if (live && i == 0) {
        double s = 0.0;
        for (int k = 0; k < A; ++k) s += lp_row[rl * A + k];
        logp[b] = (float)s;
    }
}

__global__ void beta_bwd_kernel(const float *__restrict__ dX, int n_nets, int64_t ldx, int64_t sX, int64_t col0,
                                const float *__restrict__ vec, int64_t ld_vec, const float *__restrict__ xs, int n_rows,
                                int A, const float *__restrict__ log_alpha, int use_entropy, float inv_members,
                                int data_action, float *__restrict__ d_vec, int64_t ld_dvec) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_rows * A) return;
    const int b = idx / A, i = idx - b * A;
    // dL / d log pi_b
    float c;
    if (data_action) c = inv_members / (float)n_rows;
    else c = use_entropy ? expf(log_alpha[0]) * inv_members / (float)n_rows : 0.0f;
    float g = 0.0f;   // dL / da
    if (!data_action)
        for (int j = 0; j < n_nets; ++j) g += dX[j * sX + (int64_t)b * ldx + col0 + i];
    const float va = vec[(int64_t)b * ld_vec + i], vb = vec[(int64_t)b * ld_vec + A + i];
    const float al = 1.0f + softplus20(va), be = 1.0f + softplus20(vb);
    const float am1 = al - 1.0f, bm1 = be - 1.0f;
    const float x = xs[(int64_t)b * A + i], omx = 1.0f - x;
    const double X = x, OMX = omx, AL = al, BE = be, TOT = AL + BE;
    double dal = 0.0, dbe = 0.0;
    if (c != 0.0f) {
        // direct dependence of the log-density on the concentrations (xlogy's gradient is 0 where alpha - 1 == 0)
        const double psi_t = digamma_d(TOT);
        dal = (double)c * ((am1 != 0.0f ? log(X) : 0.0) + psi_t - digamma_d(AL));
        dbe = (double)c * ((bm1 != 0.0f ? log(OMX) : 0.0) + psi_t - digamma_d(BE));
    }
    if (!data_action) {
        // through the sample: torch's _Dirichlet_backward on [x, 1 - x] with the upstream gradient on x only
        const double dx = 2.0 * (double)g + (double)c * ((double)am1 / X - (double)bm1 / OMX);
        dal += dx * dirichlet_grad_one(X, AL, TOT) * OMX;
        dbe -= dx * dirichlet_grad_one(OMX, BE, TOT) * X;
    }
    d_vec[(int64_t)b * ld_dvec + i] = softplus20_bwd(va, (float)dal);
    d_vec[(int64_t)b * ld_dvec + A + i] = softplus20_bwd(vb, (float)dbe);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int ssac_beta_fwd(const float *vec, int64_t ld_vec, int n_rows, int act_dim, int mode, const float *x_in,
                             int64_t ld_x_in, const ssac_rng *rng, float *act_dst, int64_t ld_act, int64_t act_col0,
                             float *logp, float *x_save, void *stream) {
    if (n_rows <= 0) return 0;
    if (!vec || act_dim < 1 || act_dim > BETA_THREADS || ld_vec < 2 * act_dim)
        return ssac_fail("ssac_beta_fwd: bad sizes");
    if (mode != SSAC_BETA_SAMPLE && mode != SSAC_BETA_MEAN && mode != SSAC_BETA_GIVEN)
        return ssac_fail("ssac_beta_fwd: unknown mode");
    if (mode == SSAC_BETA_MEAN && !act_dst) return ssac_fail("ssac_beta_fwd: mean mode needs act_dst");
    if (mode == SSAC_BETA_GIVEN && !x_in) return ssac_fail("ssac_beta_fwd: given-action mode needs x_in");
    if (mode == SSAC_BETA_SAMPLE && !x_in && !rng) return ssac_fail("ssac_beta_fwd: sample mode needs x_in or rng");
    if (x_in && ld_x_in < act_dim) return ssac_fail("ssac_beta_fwd: ld_x_in < act_dim");
    if (act_dst && ld_act < act_col0 + act_dim) return ssac_fail("ssac_beta_fwd: ld_act too small");
    const int rows_per_block = BETA_THREADS / act_dim;
    const RngArgs r = rng ? RngArgs{rng->seed, rng->counter, rng->offset} : RngArgs{0, nullptr, 0};
    SSAC_LAUNCH(beta_fwd_kernel, dim3((n_rows + rows_per_block - 1) / rows_per_block), dim3(rows_per_block * act_dim), 0,
                ST, vec, ld_vec, n_rows, act_dim, rows_per_block, mode, x_in, ld_x_in, r, act_dst, ld_act, act_col0, logp,
                x_save);
    return ssac_check_launch("beta_fwd");
}

extern "C" int ssac_beta_bwd(const float *dX, int n_nets, int64_t ldx, int64_t x_net_stride, int64_t act_col0,
                             const float *vec, int64_t ld_vec, const float *x_saved, int n_rows, int act_dim,
                             const float *log_alpha, int use_entropy, float inv_members, int data_action, float *d_vec,
                             int64_t ld_dvec, void *stream) {
    if (n_rows <= 0) return 0;
    if (!vec || !x_saved || !d_vec || act_dim < 1 || ld_vec < 2 * act_dim || ld_dvec < 2 * act_dim)
        return ssac_fail("ssac_beta_bwd: bad arguments");
    if (!data_action && (!dX || n_nets < 1 || ldx < act_col0 + act_dim))
        return ssac_fail("ssac_beta_bwd: the sampled-action form needs dX");
    if (!data_action && use_entropy && !log_alpha) return ssac_fail("ssac_beta_bwd: use_entropy needs log_alpha");
    const int total = n_rows * act_dim;
    SSAC_LAUNCH(beta_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, ST, dX, n_nets, ldx, x_net_stride, act_col0,
                vec, ld_vec, x_saved, n_rows, act_dim, log_alpha, use_entropy, inv_members, data_action, d_vec, ld_dvec);
    return ssac_check_launch("beta_bwd");
}
