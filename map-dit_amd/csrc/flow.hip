// Rectified-flow (linear-interpolant / flow-matching) pointwise math: the forward process, the velocity loss with its gradient, the
// logit-normal timestep map and one evaluation of the Euler / Heun ODE sampler.  Not in the reference, whose diffusion/ package knows
// variance-preserving DDPM objectives only.
//
//   x_s = (1 - s) x0 + s eps,   velocity dx/ds = eps - x0,   s = sig[t] (fp32 [T], strictly increasing in (0, 1], uploaded once)
//
// Conventions of diffusion.hip: fp32, 256-thread blocks, per-sample reductions in a fixed order, no atomics, every per-step argument
// a device pointer (the launches replay from a hipGraph), an out-of-range index clamped and recorded for mapdit_device_error_poll.
// All four kernels are memory-bound streams: where per_sample is a multiple of 4 and every buffer is 16-byte aligned a lane moves
// 16 bytes per access (VEC = 4; four consecutive elements then lie in one sample), otherwise one element (VEC = 1).  The arithmetic
// is written per component: the build keeps packed fp32 VALU code out (csrc/Makefile).
#include <math.h>

#include "common.h"

MAPDIT_DEFINE_DEV_ERROR(flow)

namespace {

#define FLOW_MAX_T 16384

template <int VEC> struct Pack;
template <> struct Pack<1> {
    float v[1];
    __device__ __forceinline__ static Pack ld(const float* p) { Pack r; r.v[0] = *p; return r; }
    __device__ __forceinline__ void st(float* p) const { *p = v[0]; }
};
template <> struct Pack<4> {
    float v[4];
    __device__ __forceinline__ static Pack ld(const float* p) {
        const f32x4_t q = *reinterpret_cast<const f32x4_t*>(p);
        Pack r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r;
    }
    __device__ __forceinline__ void st(float* p) const {
        f32x4_t q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<f32x4_t*>(p) = q;
    }
};

// x_s = (1 - s) x0 + s eps.  A lane owns one chunk of VEC consecutive elements.
template <int VEC>
__global__ __launch_bounds__(256) void flow_q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                            const long* __restrict__ t, const float* __restrict__ sig, int T,
                                                            float* __restrict__ xt, long chunks, int per) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    const long i = c * VEC;
    const long tt = MAPDIT_CHECKED_INDEX(flow, t[i / per], T, MAPDIT_DEVERR_TIMESTEP);
    const float s = sig[tt], a = 1.f - s;
    const Pack<VEC> x = Pack<VEC>::ld(x0 + i), n = Pack<VEC>::ld(noise + i);
    Pack<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = a * x.v[k] + s * n.v[k];
    o.st(xt + i);
}

// loss[n] = mean over the sample of (v - (eps - x0))^2, v = the first C channels of the model output, and G = d loss[n] / d model
// output: 2 (v - (eps - x0)) / per on those channels, exact zeros (written) on the others.  One block per sample; a lane adds its
// own terms in index order, the 64 lanes of a wave by the xor butterfly, the four wave totals in wave order.
template <int VEC>
__global__ __launch_bounds__(256) void flow_loss_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                        const float* __restrict__ noise, float* __restrict__ loss,
                                                        float* __restrict__ G, int per, int groups) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const size_t ostride = (size_t)groups * per;
    const float inv_per = 1.f / (float)per, g2 = 2.f * inv_per;
    const float* m_n = mo + (size_t)n * ostride;
    float* g_n = G + (size_t)n * ostride;
    const float* x_n = x0 + (size_t)n * per;
    const float* e_n = noise + (size_t)n * per;
    float acc = 0.f;
    for (int e = threadIdx.x * VEC; e < per; e += 256 * VEC) {
        const Pack<VEC> m = Pack<VEC>::ld(m_n + e), x = Pack<VEC>::ld(x_n + e), z = Pack<VEC>::ld(e_n + e);
        Pack<VEC> g;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float diff = m.v[k] - (z.v[k] - x.v[k]);
            acc += diff * diff;
            g.v[k] = g2 * diff;
        }
        g.st(g_n + e);
    }
    if (groups == 2) {
        Pack<VEC> zero;
#pragma unroll
        for (int k = 0; k < VEC; ++k) zero.v[k] = 0.f;
        for (int e = threadIdx.x * VEC; e < per; e += 256 * VEC) zero.st(g_n + per + e);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[n] = (((red[0] + red[1]) + red[2]) + red[3]) * inv_per;
}

// k = min(floor(sigmoid(loc + scale z) T), T - 1) in fp64, the three roundings of the numpy expression (no fused multiply-add).  A NaN
// z (it compares false everywhere) draws index 0 and is recorded.
__global__ __launch_bounds__(256) void flow_draw_kernel(const double* __restrict__ z, double loc, double scale, int T,
                                                        long* __restrict__ t_out, long N) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double u = loc + scale * z[i];
    long k = 0;
    if (u != u) {
        g_dev_error_flow = MAPDIT_DEVERR_TIMESTEP;
    } else {
        const double p = 1.0 / (1.0 + exp(-u));                          // in [0, 1] for every u, +-inf included
        k = (long)floor(p * (double)T);
        k = k < 0 ? 0 : (k > (long)T - 1 ? (long)T - 1 : k);
    }
    t_out[i] = k;
}

// One model evaluation of the Euler / Heun plan: row = step[n] of (tau, ctab, flags), v = the first C channels of the model output,
//     out = base + c_h hist + c_v v;   sample <- out
//     predictor row (flags & 1):  hist <- v                               (base kept)
//     committing row:             base_out <- out, when base_out is given
//     pred_xstart <- x_eval - sig[tau[row]] v, when pred_xstart is given
// hist is read only where c_h != 0 (a corrector row, which follows the predictor row that wrote it): an uninitialised buffer never
// reaches a sum.  Every element is read and written by the lane that owns it, so sample may be base (a committing row), base_out may be
// base and x_eval may be base or sample: none of them is __restrict__.
template <int VEC>
__global__ __launch_bounds__(256) void flow_step_kernel(const float* __restrict__ mo, const float* x_eval, const float* base,
                                                        float* __restrict__ hist, const long* __restrict__ step,
                                                        const long* __restrict__ tau, const float* __restrict__ ctab,
                                                        const int* __restrict__ flags, int J, const float* __restrict__ sig, int T,
                                                        float* sample, float* base_out, float* pred_xstart, long chunks, int per,
                                                        int groups) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    const long i = c * VEC;
    const long n = i / per, e = i % per;
    const long r = MAPDIT_CHECKED_INDEX(flow, step[n], J, MAPDIT_DEVERR_TIMESTEP);
    const long tt = MAPDIT_CHECKED_INDEX(flow, tau[r], T, MAPDIT_DEVERR_TIMESTEP);
    const float ch = ctab[2 * r], cv = ctab[2 * r + 1];
    const bool predictor = (flags[r] & 1) != 0;
    const Pack<VEC> v = Pack<VEC>::ld(mo + n * (long)groups * per + e), b = Pack<VEC>::ld(base + i);
    Pack<VEC> h, o;
    if (ch != 0.f) {
        h = Pack<VEC>::ld(hist + i);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) h.v[k] = 0.f;
    }
    if (pred_xstart) {
        const float s = sig[tt];
        const Pack<VEC> xe = Pack<VEC>::ld(x_eval + i);
        Pack<VEC> xs;
#pragma unroll
        for (int k = 0; k < VEC; ++k) xs.v[k] = xe.v[k] - s * v.v[k];
        xs.st(pred_xstart + i);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = b.v[k] + ch * h.v[k] + cv * v.v[k];
    o.st(sample + i);
    if (predictor) v.st(hist + i);
    else if (base_out && base_out != sample) o.st(base_out + i);
}

int check_T(const char* who, int T) {
    if (T < 1 || T > FLOW_MAX_T) {
        mapdit_set_error("%s: T=%d timesteps unsupported (1 <= T <= %d)", who, T, FLOW_MAX_T);
        return MAPDIT_ERR_ARG;
    }
    return MAPDIT_OK;
}

// byte ranges [a, a + na) and [b, b + nb) share a byte (a null pointer overlaps nothing)
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mapdit_flow_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sig, int T, float* xt, int N,
                                    int per_sample, void* stream) {
    MD_CHECK(x0 && noise && t && sig && xt && N > 0 && per_sample > 0, "flow_q_sample: null/empty argument");
    if (check_T("flow_q_sample", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    const size_t bytes = (size_t)N * per_sample * sizeof(float);
    MD_CHECK(!overlap(xt, bytes, x0, bytes) && !overlap(xt, bytes, noise, bytes), "flow_q_sample: overlapping arguments (xt must not overlap x0 / noise)");
    const long total = (long)N * per_sample;
    if (per_sample % 4 == 0 && aligned16(x0) && aligned16(noise) && aligned16(xt)) {
        hipLaunchKernelGGL(flow_q_sample_kernel<4>, dim3(cdiv(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, x0, noise, (const long*)t,
                           sig, T, xt, total / 4, per_sample);
    } else {
        hipLaunchKernelGGL(flow_q_sample_kernel<1>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x0, noise, (const long*)t, sig,
                           T, xt, total, per_sample);
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_flow_loss_fwd(const float* model_out, const float* x0, const float* noise, float* loss, float* G, int N,
                                    int per_sample, int groups, void* stream) {
    MD_CHECK(model_out && x0 && noise && loss && G && N > 0 && per_sample > 0, "flow_loss_fwd: null/empty argument");
    MD_CHECK(groups == 1 || groups == 2, "flow_loss_fwd: groups=%d must be 1 (C output channels) or 2 (2C, the second C ignored)", groups);
    const size_t bytes = (size_t)N * per_sample * sizeof(float), obytes = bytes * groups;
    MD_CHECK(!overlap(G, obytes, model_out, obytes) && !overlap(G, obytes, x0, bytes) && !overlap(G, obytes, noise, bytes) &&
                 !overlap(G, obytes, loss, (size_t)N * sizeof(float)) && !overlap(loss, (size_t)N * sizeof(float), model_out, obytes) &&
                 !overlap(loss, (size_t)N * sizeof(float), x0, bytes) && !overlap(loss, (size_t)N * sizeof(float), noise, bytes),
             "flow_loss_fwd: overlapping arguments (G and loss must not overlap the inputs or each other)");
    if (per_sample % 4 == 0 && aligned16(model_out) && aligned16(x0) && aligned16(noise) && aligned16(G)) {
        hipLaunchKernelGGL(flow_loss_kernel<4>, dim3(N), dim3(256), 0, (hipStream_t)stream, model_out, x0, noise, loss, G, per_sample, groups);
    } else {
        hipLaunchKernelGGL(flow_loss_kernel<1>, dim3(N), dim3(256), 0, (hipStream_t)stream, model_out, x0, noise, loss, G, per_sample, groups);
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_flow_draw_timesteps(const double* z, double loc, double scale, int T, int64_t* t_out, long N, void* stream) {
    MD_CHECK(z && t_out && N >= 1, "flow_draw_timesteps: null/empty argument");
    if (check_T("flow_draw_timesteps", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(isfinite(loc) && isfinite(scale) && scale > 0.0, "flow_draw_timesteps: loc=%g must be finite and scale=%g finite and positive", loc, scale);
    MD_CHECK(((uintptr_t)z & 7) == 0 && ((uintptr_t)t_out & 7) == 0, "flow_draw_timesteps: unaligned pointer");
    MD_CHECK(!overlap(z, (size_t)N * 8, t_out, (size_t)N * 8), "flow_draw_timesteps: overlapping arguments (t_out must not overlap z)");
    MD_CHECK((N + 255) / 256 <= 0x7fffffffL, "flow_draw_timesteps: N=%ld draws exceed one launch", N);
    hipLaunchKernelGGL(flow_draw_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, loc, scale, T, (long*)t_out, N);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_flow_step(const float* model_out, const float* x_eval, const float* base, float* hist, const int64_t* step,
                                const int64_t* tau, const float* ctab, const int* flags, int J, const float* sig, int T, float* sample,
                                float* base_out, float* pred_xstart, int N, int per_sample, int groups, void* stream) {
    MD_CHECK(model_out && base && hist && step && tau && ctab && flags && sig && sample && N > 0 && per_sample > 0 && J > 0,
             "flow_step: null/empty argument");
    MD_CHECK(!pred_xstart || x_eval, "flow_step: pred_xstart needs x_eval (null)");
    if (check_T("flow_step", T) != MAPDIT_OK) return MAPDIT_ERR_ARG;
    MD_CHECK(groups == 1 || groups == 2, "flow_step: groups=%d must be 1 (C output channels) or 2 (2C, the second C ignored)", groups);
    const size_t bytes = (size_t)N * per_sample * sizeof(float), obytes = bytes * groups;
    // an output may coincide with a buffer of x's shape where the contract says so (the owning lane reads before it writes); every other
    // overlap, a partial one included, is refused
    auto clash = [&](const void* a, const void* b, bool may_coincide) { return overlap(a, bytes, b, bytes) && !(may_coincide && a == b); };
    MD_CHECK(!overlap(hist, bytes, model_out, obytes) && !clash(hist, x_eval, false) && !clash(hist, base, false) && !clash(hist, sample, false) &&
                 !clash(hist, base_out, false) && !clash(hist, pred_xstart, false),
             "flow_step: overlapping arguments (hist must not overlap anything else)");
    MD_CHECK(!overlap(sample, bytes, model_out, obytes) && !overlap(base_out, bytes, model_out, obytes) && !overlap(pred_xstart, bytes, model_out, obytes) &&
                 !clash(sample, base, true) && !clash(sample, x_eval, true) && !clash(base_out, base, true) && !clash(base_out, x_eval, true) &&
                 !clash(base_out, sample, true) && !clash(pred_xstart, base, false) && !clash(pred_xstart, x_eval, false) &&
                 !clash(pred_xstart, sample, false) && !clash(pred_xstart, base_out, false),
             "flow_step: overlapping arguments (sample / base_out may coincide with base or x_eval; nothing else may overlap)");
    const long total = (long)N * per_sample;
    const bool vec = per_sample % 4 == 0 && aligned16(model_out) && aligned16(base) && aligned16(hist) && aligned16(sample) &&
                     aligned16(x_eval) && aligned16(base_out) && aligned16(pred_xstart);
    if (vec) {
        hipLaunchKernelGGL(flow_step_kernel<4>, dim3(cdiv(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x_eval, base, hist,
                           (const long*)step, (const long*)tau, ctab, flags, J, sig, T, sample, base_out, pred_xstart, total / 4, per_sample, groups);
    } else {
        hipLaunchKernelGGL(flow_step_kernel<1>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x_eval, base, hist,
                           (const long*)step, (const long*)tau, ctab, flags, J, sig, T, sample, base_out, pred_xstart, total, per_sample, groups);
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
