// Loss-aware timestep sampling on the device (reference diffusion/timestep_sampler.py): the loss history of
// LossSecondMomentResampler, its probability table, the draw of np.random.choice(p=...) and the importance weights.
//
// The reference keeps the history in host numpy and reads every timestep and every loss of a batch back with .item()
// (timestep_sampler.py:99-102).  Here the state stays on the device and nothing is read back:
//   hist   fp64 [T][H]   a row holds the last H losses of its timestep in chronological order (the reference's layout)
//   counts int32 [T]     how many slots of the row are filled
//   prob   fp64 [T]      the sampling distribution          cdf  fp64 [T]   its normalised running sum
// Every value that decides a probability is fp64 and every sum has a fixed order (a lane's own terms in index order, then
// the lanes' totals by a scan through LDS); there are no atomics: two runs give the same bits.
#include <math.h>

#include "common.h"

// (w / sum) * (1 - u) + u / T is three roundings in the reference (timestep_sampler.py:134-136): no fused multiply-add here
#pragma clang fp contract(off)

MAPDIT_DEFINE_DEV_ERROR(tsampler)

namespace {

#define TS_MAX_T 16384
#define TS_MAX_H 64
#define TS_UPD_LANES 256
#define TS_TAB_LANES 1024

// update_with_all_losses (timestep_sampler.py:139-147) over the M entries IN INDEX ORDER.  Lane = one timestep: it walks the
// whole batch, staged through LDS 256 entries at a time (every lane reads the same LDS word: a broadcast), and applies the
// entries that name its timestep to its own row - entries of one timestep land in index order, rows of different timesteps
// do not interact.  Two deviations from the reference, both decided while an entry is staged (it then names no row):
//   t outside [0, T)   the reference indexes numpy with it (IndexError, or the wrong row for a negative t); skipped and
//                      recorded for mapdit_device_error_poll
//   loss not finite    the reference stores it and every later weights() is NaN for H further losses of that timestep;
//                      skipped (an fp16 step that overflowed is refused by the optimiser guard as well)
__global__ __launch_bounds__(TS_UPD_LANES) void tsampler_update_kernel(double* __restrict__ hist, int* __restrict__ counts, int T, int H,
                                                                       const long* __restrict__ ts, const float* __restrict__ losses, long M) {
    __shared__ int s_t[TS_UPD_LANES];
    __shared__ float s_l[TS_UPD_LANES];
    const int lane = threadIdx.x;
    const int mine = blockIdx.x * TS_UPD_LANES + lane;
    const bool own = mine < T;
    double* row = hist + (size_t)(own ? mine : 0) * H;
    int cnt = own ? counts[mine] : 0;
    cnt = cnt < 0 ? 0 : (cnt > H ? H : cnt);                            // a count the kernel did not write never indexes past the row
    const int cnt0 = cnt;
    bool touched = false;
    for (long base = 0; base < M; base += TS_UPD_LANES) {
        const long i = base + lane;
        int st = -1;
        float sl = 0.f;
        if (i < M) {
            const long t = ts[i];
            sl = losses[i];
            if (t < 0 || t >= (long)T) {
                g_dev_error_tsampler = MAPDIT_DEVERR_SAMPLER_T;         // (every workgroup stores the same word)
            } else if (isfinite(sl)) {
                st = (int)t;
            }
        }
        __syncthreads();                                                // the previous chunk has been consumed
        s_t[lane] = st;
        s_l[lane] = sl;
        __syncthreads();
        const int n = (int)(M - base < TS_UPD_LANES ? M - base : TS_UPD_LANES);
        if (own) {
            for (int k = 0; k < n; ++k) {
                if (s_t[k] != mine) continue;
                const double v = (double)s_l[k];
                if (cnt < H) {
                    row[cnt++] = v;
                } else {                                                // shift out the oldest loss term
                    for (int j = 0; j + 1 < H; ++j) row[j] = row[j + 1];
                    row[H - 1] = v;
                }
                touched = true;
            }
        }
    }
    if (own && touched && cnt != cnt0) counts[mine] = cnt;
}

// Exclusive scan of one fp64 value per lane over the 1,024 lanes of the workgroup in a fixed order: lane 0 of each wave adds its wave's
// 64 values one after the other, lane 0 of the workgroup the 16 wave totals.  A lane receives *wexcl = the sum of the lanes before it in
// its wave and *woff = the sum of the waves before its own; *total = the sum over all lanes.  With running sums formed as
// woff + (wexcl + r) the value a lane ends on IS the value the next lane starts from, so the sums are non-decreasing for non-negative
// terms and the last one equals *total bit for bit.  buf holds 1,024 + 17 doubles.
__device__ __forceinline__ void block_scan(double v, double* buf, double* wexcl, double* woff, double* total) {
    const int lane = threadIdx.x;
    double* wtot = buf + TS_TAB_LANES;
    __syncthreads();                                                    // buf may still be read from an earlier scan
    buf[lane] = v;
    __syncthreads();
    if ((lane & 63) == 0) {
        double a = 0.0;
        for (int k = 0; k < 64; ++k) {
            const double x = buf[lane + k];
            buf[lane + k] = a;
            a += x;
        }
        wtot[lane >> 6] = a;
    }
    __syncthreads();
    if (lane == 0) {
        double a = 0.0;
        for (int w = 0; w < TS_TAB_LANES / 64; ++w) {
            const double x = wtot[w];
            wtot[w] = a;
            a += x;
        }
        wtot[TS_TAB_LANES / 64] = a;
    }
    __syncthreads();
    *wexcl = buf[lane];
    *woff = wtot[lane >> 6];
    *total = wtot[TS_TAB_LANES / 64];
}
#define TS_SCAN_DOUBLES (TS_TAB_LANES + TS_TAB_LANES / 64 + 1)

// prob holds the unnormalised distribution; cdf = cumsum(prob) / cumsum(prob)[T - 1]: what np.random.choice(p=prob) builds
// internally (mtrand: cdf = p.cumsum(); cdf /= cdf[-1]); cdf[T - 1] is exactly 1.  A lane owns the `per` consecutive entries from
// lane * per on, in every pass of the kernels below: it re-reads only what it wrote itself.
__device__ __forceinline__ void finish_table(const double* prob, double* cdf, int T, int per, double* buf) {
    const int lo = threadIdx.x * per, hi = lo + per < T ? lo + per : T;
    double run = 0.0, wexcl, woff, total;
    for (int i = lo; i < hi; ++i) run += prob[i];
    block_scan(run, buf, &wexcl, &woff, &total);
    double r = 0.0;
    for (int i = lo; i < hi; ++i) {
        r += prob[i];
        cdf[i] = (woff + (wexcl + r)) / total;
    }
}

// weights() of LossSecondMomentResampler (timestep_sampler.py:130-137) and the table of ScheduleSampler.sample (:53-54).
// One workgroup.  warmed = all(counts == H), decided here; not warmed, or a sum of the weights that is zero or not finite (the
// reference divides by it and raises inside numpy): the uniform table.
__global__ __launch_bounds__(TS_TAB_LANES) void tsampler_prepare_kernel(const double* __restrict__ hist, const int* __restrict__ counts, int T, int H,
                                                                        double uniform_prob, double* __restrict__ prob, double* __restrict__ cdf) {
    __shared__ double buf[TS_SCAN_DOUBLES];
    __shared__ int s_cold;
    const int per = (T + TS_TAB_LANES - 1) / TS_TAB_LANES;
    const int lo = threadIdx.x * per, hi = lo + per < T ? lo + per : T;
    if (threadIdx.x == 0) s_cold = 0;
    __syncthreads();
    bool cold = false;
    double run = 0.0;
    for (int i = lo; i < hi; ++i) {
        cold |= counts[i] != H;
        const double* row = hist + (size_t)i * H;
        double sq = 0.0;
        for (int j = 0; j < H; ++j) sq += row[j] * row[j];
        const double w = sqrt(sq / (double)H);
        prob[i] = w;
        run += w;
    }
    if (cold) s_cold = 1;                                               // (every lane that stores, stores the same word)
    double wexcl, woff, total;
    block_scan(run, buf, &wexcl, &woff, &total);                        // (its barriers publish s_cold)
    const bool uniform = s_cold != 0 || !(total > 0.0) || !isfinite(total);
    const double flat = 1.0 / (double)T, keep = 1.0 - uniform_prob, mix = uniform_prob / (double)T;
    for (int i = lo; i < hi; ++i) {
        double p = prob[i] / total;
        p = p * keep;
        prob[i] = uniform ? flat : p + mix;
    }
    finish_table(prob, cdf, T, per, buf);
}

// The same table from a caller's weight vector (ScheduleSampler.sample with a subclass's weights()).  The reference asks for
// positive weights (timestep_sampler.py:40-41) and np.random.choice raises on a negative or NaN probability; here a weight that
// is <= 0 or not finite is recorded for mapdit_device_error_poll and the table is the uniform one.
__global__ __launch_bounds__(TS_TAB_LANES) void tsampler_prepare_weights_kernel(const double* __restrict__ weights, int T, double* __restrict__ prob,
                                                                                double* __restrict__ cdf) {
    __shared__ double buf[TS_SCAN_DOUBLES];
    __shared__ int s_bad;
    const int per = (T + TS_TAB_LANES - 1) / TS_TAB_LANES;
    const int lo = threadIdx.x * per, hi = lo + per < T ? lo + per : T;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    double run = 0.0;
    for (int i = lo; i < hi; ++i) {
        const double w = weights[i];
        bad |= !(w > 0.0) || !isfinite(w);
        run += w;
    }
    if (bad) s_bad = 1;
    double wexcl, woff, total;
    block_scan(run, buf, &wexcl, &woff, &total);                        // (its barriers publish s_bad)
    const bool uniform = s_bad != 0 || !(total > 0.0) || !isfinite(total);
    if (uniform && threadIdx.x == 0) g_dev_error_tsampler = MAPDIT_DEVERR_WEIGHT;
    const double flat = 1.0 / (double)T;
    for (int i = lo; i < hi; ++i) prob[i] = uniform ? flat : weights[i] / total;
    finish_table(prob, cdf, T, per, buf);
}

// np.random.choice(T, p=prob) for given uniforms (mtrand: cdf.searchsorted(u, side="right")) and the importance weights
// 1 / (T p[t]) of ScheduleSampler.sample (timestep_sampler.py:55-58).  A NaN uniform compares false everywhere and draws 0.
__global__ __launch_bounds__(256) void tsampler_draw_kernel(const double* __restrict__ prob, const double* __restrict__ cdf, int T,
                                                            const double* __restrict__ u, long* __restrict__ t_out, float* __restrict__ w_out, long N) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double x = u[i];
    int lo = 0, hi = T;                                                 // #{k : cdf[k] <= x} lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= x) lo = mid + 1; else hi = mid;
    }
    const int t = lo < T - 1 ? lo : T - 1;
    t_out[i] = t;
    w_out[i] = (float)(1.0 / ((double)T * prob[t]));
}

int check_T(const char* who, int T) {
    if (T < 1 || T > TS_MAX_T) {
        mapdit_set_error("%s: T=%d timesteps unsupported (1 <= T <= %d)", who, T, TS_MAX_T);
        return MAPDIT_ERR_ARG;
    }
    return MAPDIT_OK;
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" int mapdit_tsampler_update(double* hist, int* counts, int T, int H, const int64_t* ts, const float* losses, long M, void* stream) {
    if (check_T("tsampler_update", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(H >= 1 && H <= TS_MAX_H, "tsampler_update: H=%d history slots per timestep unsupported (1 <= H <= %d)", H, TS_MAX_H);
    MD_CHECK(M >= 1, "tsampler_update: M=%ld entries (M >= 1)", M);
    MD_CHECK(hist && counts && ts && losses, "tsampler_update: null pointer (hist, counts, ts, losses)");
    MD_CHECK(aligned8(hist) && aligned8(ts) && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)losses & 3) == 0, "tsampler_update: unaligned pointer");
    hipLaunchKernelGGL(tsampler_update_kernel, dim3(cdiv(T, TS_UPD_LANES)), dim3(TS_UPD_LANES), 0, (hipStream_t)stream, hist, counts, T, H,
                       (const long*)ts, losses, M);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_tsampler_prepare(const double* hist, const int* counts, int T, int H, double uniform_prob, double* prob, double* cdf,
                                       void* stream) {
    if (check_T("tsampler_prepare", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(H >= 1 && H <= TS_MAX_H, "tsampler_prepare: H=%d history slots per timestep unsupported (1 <= H <= %d)", H, TS_MAX_H);
    MD_CHECK(uniform_prob >= 0.0 && uniform_prob <= 1.0, "tsampler_prepare: uniform_prob=%g must lie in [0, 1]", uniform_prob);   // (false for NaN)
    MD_CHECK(hist && counts && prob && cdf, "tsampler_prepare: null pointer (hist, counts, prob, cdf)");
    MD_CHECK(aligned8(hist) && aligned8(prob) && aligned8(cdf) && ((uintptr_t)counts & 3) == 0, "tsampler_prepare: unaligned pointer");
    hipLaunchKernelGGL(tsampler_prepare_kernel, dim3(1), dim3(TS_TAB_LANES), 0, (hipStream_t)stream, hist, counts, T, H, uniform_prob, prob, cdf);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_tsampler_prepare_weights(const double* weights, int T, double* prob, double* cdf, void* stream) {
    if (check_T("tsampler_prepare_weights", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(weights && prob && cdf, "tsampler_prepare_weights: null pointer (weights, prob, cdf)");
    MD_CHECK(aligned8(weights) && aligned8(prob) && aligned8(cdf), "tsampler_prepare_weights: unaligned pointer");
    MD_CHECK(weights != prob && weights != cdf, "tsampler_prepare_weights: weights must not alias prob / cdf");
    hipLaunchKernelGGL(tsampler_prepare_weights_kernel, dim3(1), dim3(TS_TAB_LANES), 0, (hipStream_t)stream, weights, T, prob, cdf);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_tsampler_draw(const double* prob, const double* cdf, int T, const double* u, int64_t* t_out, float* w_out, long N,
                                    void* stream) {
    if (check_T("tsampler_draw", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(N >= 1, "tsampler_draw: N=%ld draws (N >= 1)", N);
    MD_CHECK(prob && cdf && u && t_out && w_out, "tsampler_draw: null pointer (prob, cdf, u, t_out, w_out)");
    MD_CHECK(aligned8(prob) && aligned8(cdf) && aligned8(u) && aligned8(t_out) && ((uintptr_t)w_out & 3) == 0, "tsampler_draw: unaligned pointer");
    MD_CHECK((N + 255) / 256 <= 0x7fffffffL, "tsampler_draw: N=%ld draws exceed one launch", N);
    hipLaunchKernelGGL(tsampler_draw_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, prob, cdf, T, u, (long*)t_out,
                       w_out, N);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
