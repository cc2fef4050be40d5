// Replay gather for observations that are SEVERAL vector arrays laid side by side (ssac_concat in include/ssac_hip.h):
// what ssac_gather_transition writes, with the state columns [key_0 | key_1 | ... | key_{K-1}] for both s and s'.
//
// Byte / row work like the rest of the sample path: one element per thread per trip, consecutive threads walk one output
// row, so stores are coalesced and the loads are coalesced inside each key's run of columns.  The launch is a few
// thousand elements and latency-bound; the key of a column is found by comparing it with the (at most 8) prefix offsets
// that sit in the argument block -- no table in memory, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "ssac_begin.h"
#include "ssac_internal.h"

namespace {

// the launch's copy of the table: prefix offsets instead of widths; off[j] = S for every j >= n_keys, so that
// "number of offsets a column has reached" is its key whatever n_keys is
struct ConcatArgs {
    const void *s[SSAC_MAX_OBS_KEYS];
    const void *s1[SSAC_MAX_OBS_KEYS];
    int64_t off[SSAC_MAX_OBS_KEYS + 1];   // off[0] = 0
    int32_t u8[SSAC_MAX_OBS_KEYS];        // 1: the key's arrays are uint8 (cast to float)
};

__device__ __forceinline__ float concat_load(const void *p, int u8, int64_t i) {
    return u8 ? (float)reinterpret_cast<const uint8_t *>(p)[i] : reinterpret_cast<const float *>(p)[i];
}

// One row of work = S + nA + nS1 + nR + nD elements: [s | a | s' | r | d], a section of width 0 being one whose
// destination the caller left out (only the idx == NULL form may).
__global__ void gather_concat_kernel(ConcatArgs t, int64_t S, const float *__restrict__ act, int64_t a_elems, int64_t nA,
                                     int64_t nS1, int nR, const float *__restrict__ rew,
                                     const uint8_t *__restrict__ done, const int64_t *__restrict__ idx, int n_rows,
                                     float *__restrict__ xsa, int64_t ld_x, float *__restrict__ x1sa, int64_t ld_x1,
                                     float *__restrict__ rew_out, float *__restrict__ done_out, int64_t per_row,
                                     const ssac_feed *feed, float *logs, int n_logs, ssac_adam_ctl *ctl) {
    if (feed) {
        // first launch of a recorded update (as gather_transition_kernel): indices from this update's slot of the input
        // ring, and workgroup 0 does ssac_begin_update's work
        const ssac_feed f = *feed;
        idx = reinterpret_cast<const int64_t *>(feed_slot(f));
        if (blockIdx.x == 0) {
            feed_pull(f);
            if ((int)threadIdx.x < n_logs) logs[threadIdx.x] = 0.0f;
            if (threadIdx.x == 0 && ctl) adam_refresh(ctl, ctl->step + 1);
        }
    }
    const int64_t total = (int64_t)n_rows * per_row;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        int64_t c = i - r * per_row;
        const int64_t src = idx ? idx[r] : r;
        const bool in_s = c < S;
        if (in_s || ((c -= S + nA) >= 0 && c < nS1)) {
            // a state column of s (-> xsa) or of s' (-> x1sa): its key, then the element of that key's row
            int k = 0;
#pragma unroll
            for (int j = 1; j < SSAC_MAX_OBS_KEYS; ++j) k += c >= t.off[j] ? 1 : 0;
            const int64_t w = t.off[k + 1] - t.off[k];
            const float v = concat_load(in_s ? t.s[k] : t.s1[k], t.u8[k], src * w + (c - t.off[k]));
            if (in_s) xsa[r * ld_x + c] = v;
            else x1sa[r * ld_x1 + c] = v;
        } else if (c < 0) {
            c += nA;   // the action columns
            xsa[r * ld_x + S + c] = act[src * a_elems + c];
        } else if ((c -= nS1) < nR) {
            rew_out[r] = rew[src];
        } else {
            done_out[r] = (float)done[src];
        }
    }
}

int refuse(const char *who, const char *why) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return ssac_fail(msg);
}

int gather_concat_impl(const char *who, const ssac_concat *table, const float *act, int64_t a_elems, const float *rew,
                       const uint8_t *done, const int64_t *idx, int n_rows, float *xsa, int64_t ld_x, float *x1sa,
                       int64_t ld_x1, float *rew_out, float *done_out, const ssac_feed *feed, float *logs, int n_logs,
                       ssac_adam_ctl *ctl, void *stream) {
    if (!table) return refuse(who, "needs a key table");
    const int K = table->n_keys;
    if (K < 1 || K > SSAC_MAX_OBS_KEYS) return refuse(who, "the key count must be 1 .. SSAC_MAX_OBS_KEYS");
    if (!xsa) return refuse(who, "needs xsa");
    const bool indexed = idx != nullptr || feed != nullptr;
    // rows through an index vector: the whole transition; row r = row r (idx NULL): every part but s -> xsa may be left out
    const bool want_s1 = indexed || x1sa != nullptr;
    ConcatArgs t;
    int64_t S = 0;
    t.off[0] = 0;
    for (int k = 0; k < K; ++k) {
        const ssac_concat_key &e = table->key[k];
        if (e.dtype != 0 && e.dtype != 1) return refuse(who, "unsupported key dtype");
        if (e.elems < 1) return refuse(who, "a key needs elems >= 1");
        if (!e.s || (want_s1 && !e.s1)) return refuse(who, "a key's source array is NULL");
        t.s[k] = e.s; t.s1[k] = e.s1; t.u8[k] = e.dtype;
        S += e.elems;
        t.off[k + 1] = S;
    }
    for (int k = K; k < SSAC_MAX_OBS_KEYS; ++k) {
        t.s[k] = t.s1[k] = nullptr; t.u8[k] = 0;
        t.off[k + 1] = S;
    }
    if (a_elems < 0) return refuse(who, "a_elems < 0");
    if (indexed && !(x1sa && act && rew && done && rew_out && done_out))
        return refuse(who, "an indexed gather writes the whole transition: a source or destination is NULL");
    if ((rew == nullptr) != (rew_out == nullptr) || (done == nullptr) != (done_out == nullptr))
        return refuse(who, "rew / done need both their source and their destination");
    const int64_t nA = act ? a_elems : 0;
    if (ld_x < S + nA) return refuse(who, "ld_x < S + A");
    if (want_s1 && ld_x1 < S) return refuse(who, "ld_x1 < S");
    if (n_logs > 256) return refuse(who, "log block too large");
    if (n_rows <= 0) return 0;
    const int64_t nS1 = want_s1 ? S : 0;
    const int nR = rew ? 1 : 0;
    const int64_t per_row = S + nA + nS1 + nR + (done ? 1 : 0);
    const int64_t total = (int64_t)n_rows * per_row;
    const int64_t blocks = (total + 255) / 256;
    SSAC_LAUNCH(gather_concat_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, t,
                S, act, a_elems, nA, nS1, nR, rew, done, idx, n_rows, xsa, ld_x, x1sa, ld_x1, rew_out, done_out, per_row,
                feed, logs, n_logs, ctl);
    return ssac_check_launch("gather_concat");
}

}  // namespace

extern "C" int ssac_gather_concat(const ssac_concat *table, const float *act, int64_t a_elems, const float *rew,
                                  const uint8_t *done, const int64_t *idx, int n_rows, float *xsa, int64_t ld_x,
                                  float *x1sa, int64_t ld_x1, float *rew_out, float *done_out, void *stream) {
    return gather_concat_impl("ssac_gather_concat", table, act, a_elems, rew, done, idx, n_rows, xsa, ld_x, x1sa, ld_x1,
                              rew_out, done_out, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int ssac_gather_concat_begin(const ssac_concat *table, const float *act, int64_t a_elems, const float *rew,
                                        const uint8_t *done, int n_rows, float *xsa, int64_t ld_x, float *x1sa,
                                        int64_t ld_x1, float *rew_out, float *done_out, const ssac_feed *feed, float *logs,
                                        int n_logs, ssac_adam_ctl *ctl, void *stream) {
    if (!feed) return refuse("ssac_gather_concat_begin", "needs a feed");
    if (n_logs > 0 && !logs) return refuse("ssac_gather_concat_begin", "n_logs > 0 without a log block");
    return gather_concat_impl("ssac_gather_concat_begin", table, act, a_elems, rew, done, nullptr, n_rows, xsa, ld_x, x1sa,
                              ld_x1, rew_out, done_out, feed, logs, n_logs, ctl, stream);
}
