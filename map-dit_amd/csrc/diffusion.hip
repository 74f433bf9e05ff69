// Gaussian-diffusion pointwise math: q_sample, the MSE + variational-bound training loss
// with its gradient, and the fused p_mean_variance + p_sample update.  Schedule tables live on the device as
// fp32 arrays (uploaded once), replacing the per-call numpy uploads of reference gaussian_diffusion.py:861-873.
//
// Table layout `tab` = 8 rows of `nsteps` floats:
//   0 sqrt_alphas_cumprod        1 sqrt_one_minus_alphas_cumprod   2 sqrt_recip_alphas_cumprod
//   3 sqrt_recipm1_alphas_cumprod 4 posterior_log_variance_clipped  5 log(betas)
//   6 posterior_mean_coef1        7 posterior_mean_coef2
#include "common.h"

MAPDIT_DEFINE_DEV_ERROR(diffusion)

namespace {

#define INV_LN2 1.44269504088896341f

// x_t = sqrt(acp[t]) x0 + sqrt(1-acp[t]) noise            (reference gaussian_diffusion.py:215-230)
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const long* __restrict__ t,
                                const float* __restrict__ tab, int nsteps, float* __restrict__ xt, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[i / per], nsteps, MAPDIT_DEVERR_TIMESTEP);
    xt[i] = tab[tt] * x0[i] + tab[nsteps + tt] * noise[i];
}

__device__ __forceinline__ float cdf_approx(float x, float* dcdf) {
    // diffusion_utils.py:39-44
    const float k = 0.79788456080286536f;   // sqrt(2/pi)
    const float u = k * (x + 0.044715f * x * x * x);
    const float th = tanhf(u);
    *dcdf = 0.5f * (1.f - th * th) * k * (1.f + 3.f * 0.044715f * x * x);
    return 0.5f * (1.f + th);
}

// training_losses, MSE + LEARNED_RANGE branch (reference gaussian_diffusion.py:715-787, 682-713,
// diffusion_utils.py:10-37,62-88).  One block per sample.  Writes mse[n], vb[n], loss[n] and
// G[n, 0:C] = d mse[n] / d eps,  G[n, C:2C] = d vb[n] / d v  (the vb term sees eps detached).
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                 const float* __restrict__ xt, const float* __restrict__ noise,
                                                 const long* __restrict__ t, const float* __restrict__ tab, int nsteps,
                                                 float* __restrict__ mse, float* __restrict__ vb, float* __restrict__ loss,
                                                 float* __restrict__ G, int per /* C*H*W */) {
    __shared__ float red[2][4];
    const int n = blockIdx.x;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const float ra = tab[2 * nsteps + tt], rm1 = tab[3 * nsteps + tt], minlog = tab[4 * nsteps + tt],
                maxlog = tab[5 * nsteps + tt], c1 = tab[6 * nsteps + tt], c2 = tab[7 * nsteps + tt];
    const float inv_per = 1.f / (float)per;
    const bool first = tt == 0;
    float a_mse = 0.f, a_vb = 0.f;
    for (int e = threadIdx.x; e < per; e += 256) {
        const size_t ie = (size_t)n * 2 * per + e, iv = ie + per, ix = (size_t)n * per + e;
        const float eps = mo[ie], v = mo[iv], x_0 = x0[ix], x_t = xt[ix], nz = noise[ix];
        const float diff = nz - eps;
        a_mse += diff * diff;
        G[ie] = -2.f * diff * inv_per;
        const float frac = (v + 1.f) * 0.5f;
        const float lv = frac * maxlog + (1.f - frac) * minlog;
        const float xs = ra * x_t - rm1 * eps;
        const float mean = c1 * xs + c2 * x_t;
        const float tmean = c1 * x_0 + c2 * x_t;
        const float dlv_dv = 0.5f * (maxlog - minlog);
        float term, dterm_dlv;
        if (!first) {
            const float e1 = expf(minlog - lv), e2 = expf(-lv), dm = tmean - mean;
            term = 0.5f * (-1.f + lv - minlog + e1 + dm * dm * e2);
            dterm_dlv = 0.5f * (1.f - e1 - dm * dm * e2);
        } else {
            const float cx = x_0 - mean, inv = expf(-0.5f * lv);
            const float pin = inv * (cx + 1.f / 255.f), mnn = inv * (cx - 1.f / 255.f);
            float dcp, dcm;
            const float cp = cdf_approx(pin, &dcp), cm = cdf_approx(mnn, &dcm);
            float lp, dlp;   // log prob and d log prob / d lv   (d inv / d lv = -inv/2 => d pin / d lv = -pin/2)
            if (x_0 < -0.999f) {
                lp = logf(fmaxf(cp, 1e-12f));
                dlp = cp > 1e-12f ? dcp * (-0.5f * pin) / cp : 0.f;
            } else if (x_0 > 0.999f) {
                lp = logf(fmaxf(1.f - cm, 1e-12f));
                dlp = (1.f - cm) > 1e-12f ? -dcm * (-0.5f * mnn) / (1.f - cm) : 0.f;
            } else {
                const float dl = cp - cm;
                lp = logf(fmaxf(dl, 1e-12f));
                dlp = dl > 1e-12f ? (dcp * (-0.5f * pin) - dcm * (-0.5f * mnn)) / dl : 0.f;
            }
            term = -lp;
            dterm_dlv = -dlp;
        }
        a_vb += term;
        G[iv] = dterm_dlv * dlv_dv * inv_per * INV_LN2;
    }
    a_mse = wave_sum(a_mse);
    a_vb = wave_sum(a_vb);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a_mse; red[1][threadIdx.x >> 6] = a_vb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) * inv_per;
        const float b = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) * inv_per * INV_LN2;
        mse[n] = m; vb[n] = b; loss[n] = m + b;
    }
}

// dout[n, 0:C] = (gl[n]+gm[n]) G[n, 0:C];  dout[n, C:2C] = (gl[n]+gv[n]) G[n, C:2C]
__global__ void loss_bwd_kernel(const float* __restrict__ G, const float* __restrict__ gl, const float* __restrict__ gm,
                                const float* __restrict__ gv, float* __restrict__ dout, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i / (2 * per));
    const bool is_v = (i % (2 * per)) >= per;
    const float g = (gl ? gl[n] : 0.f) + (is_v ? (gv ? gv[n] : 0.f) : (gm ? gm[n] : 0.f));
    dout[i] = g * G[i];
}

// p_mean_variance + p_sample (reference gaussian_diffusion.py:254-332, 376-417) for EPSILON / LEARNED_RANGE.
// `t` holds each sample's index into the (respaced) schedule, on the device, so the launch replays from a hipGraph.
__global__ void p_sample_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ noise,
                                const long* __restrict__ t, const float* __restrict__ tab, int nsteps, int clip,
                                float* __restrict__ sample, float* __restrict__ xstart, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const float eps = mo[n * 2 * per + e], v = mo[n * 2 * per + per + e], x_t = x[i];
    const float ra = tab[2 * nsteps + tt], rm1 = tab[3 * nsteps + tt], minlog = tab[4 * nsteps + tt],
                maxlog = tab[5 * nsteps + tt], c1 = tab[6 * nsteps + tt], c2 = tab[7 * nsteps + tt];
    const float frac = (v + 1.f) * 0.5f;
    const float lv = frac * maxlog + (1.f - frac) * minlog;
    float xs = ra * x_t - rm1 * eps;
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    const float mean = c1 * xs + c2 * x_t;
    sample[i] = mean + (tt != 0 ? expf(0.5f * lv) * noise[i] : 0.f);
    if (xstart) xstart[i] = xs;
}

// DDIM step (reference gaussian_diffusion.py:513-567) and its reverse ODE step (:569-605) for EPSILON / LEARNED_RANGE models:
// x0^ from the predicted noise (clipped on request), the noise re-derived from x0^ (_predict_eps_from_xstart), then Eq. 12 of
// Song et al. 2020.  dtab = [alphas_cumprod | alphas_cumprod_prev | alphas_cumprod_next] (fp32 rows of the respaced schedule).
__global__ void ddim_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ noise,
                            const long* __restrict__ t, const float* __restrict__ tab, const float* __restrict__ dtab, int nsteps,
                            int clip, float eta, int reverse, float* __restrict__ sample, float* __restrict__ xstart, long total,
                            int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const float epsm = mo[n * 2 * per + e], x_t = x[i];
    const float ra = tab[2 * nsteps + tt], rm1 = tab[3 * nsteps + tt];
    float xs = ra * x_t - rm1 * epsm;
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    const float eps = (ra * x_t - xs) / rm1;
    float out;
    if (reverse) {
        const float abn = dtab[2 * nsteps + tt];
        out = xs * sqrtf(abn) + sqrtf(1.f - abn) * eps;
    } else {
        const float ab = dtab[tt], abp = dtab[nsteps + tt];
        const float sigma = eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
        out = xs * sqrtf(abp) + sqrtf(1.f - abp - sigma * sigma) * eps;
        if (tt != 0) out += sigma * noise[i];
    }
    sample[i] = out;
    if (xstart) xstart[i] = xs;
}

}  // namespace

extern "C" int mapdit_ddim_step(const float* model_out, const float* x, const float* noise, const int64_t* t, const float* tab,
                                const float* dtab, int nsteps, int clip_denoised, float eta, int reverse, float* sample,
                                float* pred_xstart, int N, int per_sample, void* stream) {
    MD_CHECK(model_out && x && t && tab && dtab && sample && N > 0, "ddim_step: null/empty argument");
    MD_CHECK(reverse || noise, "ddim_step: the forward step needs the noise tensor");
    MD_CHECK(!reverse || eta == 0.f, "ddim_step: the reverse ODE is deterministic (eta must be 0)");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(ddim_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, noise, (const long*)t, tab,
                       dtab, nsteps, clip_denoised, eta, reverse, sample, pred_xstart, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_q_sample(const float* x0, const float* noise, const int64_t* t, const float* tab, int nsteps, float* xt,
                               int N, int per_sample, void* stream) {
    MD_CHECK(x0 && noise && t && tab && xt && N > 0, "q_sample: null/empty argument");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(q_sample_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x0, noise, (const long*)t, tab,
                       nsteps, xt, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_loss_fwd(const float* model_out, const float* x0, const float* xt, const float* noise, const int64_t* t,
                               const float* tab, int nsteps, float* mse, float* vb, float* loss, float* G, int N, int per_sample,
                               void* stream) {
    MD_CHECK(model_out && x0 && xt && noise && t && tab && mse && vb && loss && G && N > 0, "loss_fwd: null/empty argument");
    hipLaunchKernelGGL(loss_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, model_out, x0, xt, noise, (const long*)t, tab,
                       nsteps, mse, vb, loss, G, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_loss_bwd(const float* G, const float* g_loss, const float* g_mse, const float* g_vb, float* dout, int N,
                               int per_sample, void* stream) {
    MD_CHECK(G && dout && N > 0, "loss_bwd: null/empty argument");
    const long total = (long)N * 2 * per_sample;
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, G, g_loss, g_mse, g_vb, dout,
                       total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_psample_step(const float* model_out, const float* x, const float* noise, const int64_t* t, const float* tab,
                                   int nsteps, int clip_denoised, float* sample, float* pred_xstart, int N, int per_sample,
                                   void* stream) {
    MD_CHECK(model_out && x && noise && t && tab && sample && N > 0, "psample_step: null/empty argument");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(p_sample_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, noise, (const long*)t, tab,
                       nsteps, clip_denoised, sample, pred_xstart, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Every objective create_diffusion() can build (reference gaussian_diffusion.py:203-344, 682-858): mean type EPSILON / START_X,
// variance type LEARNED_RANGE / FIXED_SMALL / FIXED_LARGE, loss MSE / RESCALED_MSE / KL / RESCALED_KL, and the bound terms of
// calc_bpd_loop.  The kernels above stay the default configuration's path; these read `tab` (8 rows, above) plus `otab`:
//   0 alphas_cumprod   1 alphas_cumprod_prev   2 alphas_cumprod_next
//   3 log(append(posterior_variance[1], betas[1:]))  (FIXED_LARGE)   4 log_one_minus_alphas_cumprod
// The model output holds 2C channels per sample for LEARNED_RANGE (mean | v) and C for the fixed variances.
namespace {

enum { OBJ_EPSILON = 0, OBJ_START_X = 1 };
enum { OBJ_LEARNED_RANGE = 0, OBJ_FIXED_SMALL = 1, OBJ_FIXED_LARGE = 2 };
enum { OBJ_MSE = 0, OBJ_RESCALED_MSE = 1, OBJ_KL = 2, OBJ_RESCALED_KL = 3 };
enum { OBJ_STEP_PSAMPLE = 0, OBJ_STEP_DDIM = 1, OBJ_STEP_DDIM_REVERSE = 2 };

struct ObjCoef {
    float ra, rm1, minlog, maxlog, c1, c2, fixlog;
};

__device__ __forceinline__ ObjCoef obj_coef(const float* __restrict__ tab, const float* __restrict__ otab, int nsteps, long tt) {
    ObjCoef c;
    c.ra = tab[2 * nsteps + tt]; c.rm1 = tab[3 * nsteps + tt]; c.minlog = tab[4 * nsteps + tt]; c.maxlog = tab[5 * nsteps + tt];
    c.c1 = tab[6 * nsteps + tt]; c.c2 = tab[7 * nsteps + tt]; c.fixlog = otab[3 * nsteps + tt];
    return c;
}

// model log-variance (p_mean_variance, :286-311) and d lv / d v (LEARNED_RANGE only; 0 for the fixed rows)
__device__ __forceinline__ float obj_logvar(int var_type, const ObjCoef& c, float v, float* dlv_dv) {
    if (var_type == OBJ_LEARNED_RANGE) {
        const float frac = (v + 1.f) * 0.5f;
        *dlv_dv = 0.5f * (c.maxlog - c.minlog);
        return frac * c.maxlog + (1.f - frac) * c.minlog;
    }
    *dlv_dv = 0.f;
    return var_type == OBJ_FIXED_SMALL ? c.minlog : c.fixlog;
}

// One element of _vb_terms_bpd (:682-713) in nats: normal_kl(true mean, true log-variance, mean, lv) for t > 0, the
// discretized-Gaussian decoder NLL at t = 0 (diffusion_utils.py:10-37, 62-88), with its derivatives wrt lv and wrt the model
// mean.  The clamps at 1e-12 pass no gradient, as loss_kernel's.
__device__ __forceinline__ float obj_vb_term(bool first, float x_0, float mean, float lv, float tmean, float minlog, float* d_lv,
                                             float* d_mean) {
    if (!first) {
        const float e1 = expf(minlog - lv), e2 = expf(-lv), dm = tmean - mean;
        *d_lv = 0.5f * (1.f - e1 - dm * dm * e2);
        *d_mean = -dm * e2;
        return 0.5f * (-1.f + lv - minlog + e1 + dm * dm * e2);
    }
    const float cx = x_0 - mean, inv = expf(-0.5f * lv);
    const float pin = inv * (cx + 1.f / 255.f), mnn = inv * (cx - 1.f / 255.f);
    float dcp, dcm;
    const float cp = cdf_approx(pin, &dcp), cm = cdf_approx(mnn, &dcm);
    // d pin / d lv = -pin/2, d pin / d mean = -inv (likewise mnn)
    float lp, dlp, dlpm;
    if (x_0 < -0.999f) {
        lp = logf(fmaxf(cp, 1e-12f));
        const bool on = cp > 1e-12f;
        dlp = on ? dcp * (-0.5f * pin) / cp : 0.f;
        dlpm = on ? dcp * (-inv) / cp : 0.f;
    } else if (x_0 > 0.999f) {
        lp = logf(fmaxf(1.f - cm, 1e-12f));
        const bool on = (1.f - cm) > 1e-12f;
        dlp = on ? -dcm * (-0.5f * mnn) / (1.f - cm) : 0.f;
        dlpm = on ? -dcm * (-inv) / (1.f - cm) : 0.f;
    } else {
        const float dl = cp - cm;
        lp = logf(fmaxf(dl, 1e-12f));
        const bool on = dl > 1e-12f;
        dlp = on ? (dcp * (-0.5f * pin) - dcm * (-0.5f * mnn)) / dl : 0.f;
        dlpm = on ? (dcp * (-inv) - dcm * (-inv)) / dl : 0.f;
    }
    *d_lv = -dlp;
    *d_mean = -dlpm;
    return -lp;
}

// Sums of up to three per-thread values over a 256-thread block; the result is valid in thread 0.
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c) {
    __shared__ float red[3][4];
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        c = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    }
}

// training_losses (:715-787) for every built objective.  One block per sample.  MSE / RESCALED_MSE: mse[n], loss[n], and with
// LEARNED_RANGE vb[n] (the vb term sees the mean channels detached; x num_timesteps/1000 for RESCALED_MSE); G[n, 0:C] = d mse / d
// model mean channels, G[n, C:2C] = d vb / d v.  KL / RESCALED_KL: loss[n] = the bound term with clip_denoised=False
// (x num_timesteps for RESCALED_KL) and G = d loss / d model output, through mean = c1 x0^ + c2 x_t and (LEARNED_RANGE) v.
__global__ __launch_bounds__(256) void obj_loss_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                     const float* __restrict__ xt, const float* __restrict__ noise,
                                                     const long* __restrict__ t, const float* __restrict__ tab,
                                                     const float* __restrict__ otab, int nsteps, int mean_type, int var_type,
                                                     int loss_type, float* __restrict__ mse, float* __restrict__ vb,
                                                     float* __restrict__ loss, float* __restrict__ G, int per) {
    const int n = blockIdx.x;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const ObjCoef c = obj_coef(tab, otab, nsteps, tt);
    const bool learned = var_type == OBJ_LEARNED_RANGE, is_kl = loss_type >= OBJ_KL, start_x = mean_type == OBJ_START_X;
    const bool need_vb = is_kl || learned;
    const float vb_scale = loss_type == OBJ_RESCALED_MSE ? (float)nsteps / 1000.f : loss_type == OBJ_RESCALED_KL ? (float)nsteps : 1.f;
    const size_t ostride = learned ? 2 * (size_t)per : (size_t)per;
    const float inv_per = 1.f / (float)per;
    const float dxs_dm = start_x ? 1.f : -c.rm1;
    const bool first = tt == 0;
    float a_mse = 0.f, a_vb = 0.f, unused = 0.f;
    for (int e = threadIdx.x; e < per; e += 256) {
        const size_t im = (size_t)n * ostride + e, iv = im + per, ix = (size_t)n * per + e;
        const float m = mo[im], x_0 = x0[ix], x_t = xt[ix];
        if (!is_kl) {
            const float diff = (start_x ? x_0 : noise[ix]) - m;
            a_mse += diff * diff;
            G[im] = -2.f * diff * inv_per;
        }
        if (need_vb) {
            float dlv_dv, d_lv, d_mean;
            const float lv = obj_logvar(var_type, c, learned ? mo[iv] : 0.f, &dlv_dv);
            const float xs = start_x ? m : c.ra * x_t - c.rm1 * m;
            const float mean = c.c1 * xs + c.c2 * x_t;
            const float tmean = c.c1 * x_0 + c.c2 * x_t;
            a_vb += obj_vb_term(first, x_0, mean, lv, tmean, c.minlog, &d_lv, &d_mean);
            if (learned) G[iv] = d_lv * dlv_dv * inv_per * INV_LN2 * vb_scale;
            if (is_kl) G[im] = d_mean * c.c1 * dxs_dm * inv_per * INV_LN2 * vb_scale;
        }
    }
    block_sum3(a_mse, a_vb, unused);
    if (threadIdx.x == 0) {
        const float b = a_vb * inv_per * INV_LN2 * vb_scale;
        if (is_kl) {
            loss[n] = b;
        } else {
            const float m = a_mse * inv_per;
            mse[n] = m;
            if (learned) vb[n] = b;
            loss[n] = learned ? m + b : m;
        }
    }
}

// dout[n, 0:C] = (gl[n]+gm[n]) G[n, 0:C];  dout[n, C:2C] = (gl[n]+gv[n]) G[n, C:2C]  (groups = 2: LEARNED_RANGE; 1: C channels)
__global__ void obj_loss_bwd_kernel(const float* __restrict__ G, const float* __restrict__ gl, const float* __restrict__ gm,
                                    const float* __restrict__ gv, float* __restrict__ dout, long total, int per, int groups) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long stride = (long)groups * per;
    const long n = i / stride;
    const bool is_v = (i % stride) >= per;
    const float g = (gl ? gl[n] : 0.f) + (is_v ? (gv ? gv[n] : 0.f) : (gm ? gm[n] : 0.f));
    dout[i] = g * G[i];
}

// p_mean_variance (:254-332) followed by p_sample (:376-417), ddim_sample (:513-567) or ddim_reverse_sample (:569-605).
// p_sample without noise (nullptr) writes the model mean.
__global__ void obj_step_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ noise,
                                const long* __restrict__ t, const float* __restrict__ tab, const float* __restrict__ otab, int nsteps,
                                int mean_type, int var_type, int clip, int mode, float eta, float* __restrict__ sample,
                                float* __restrict__ xstart, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const bool learned = var_type == OBJ_LEARNED_RANGE;
    const long ostride = learned ? 2 * (long)per : (long)per;
    const float m = mo[n * ostride + e], x_t = x[i];
    const ObjCoef c = obj_coef(tab, otab, nsteps, tt);
    float xs = mean_type == OBJ_START_X ? m : c.ra * x_t - c.rm1 * m;
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    float out;
    if (mode == OBJ_STEP_PSAMPLE) {
        out = c.c1 * xs + c.c2 * x_t;
        if (noise && tt != 0) {
            float dlv_dv;
            const float lv = obj_logvar(var_type, c, learned ? mo[n * ostride + per + e] : 0.f, &dlv_dv);
            out += expf(0.5f * lv) * noise[i];
        }
    } else {
        const float eps = (c.ra * x_t - xs) / c.rm1;          // _predict_eps_from_xstart
        if (mode == OBJ_STEP_DDIM_REVERSE) {
            const float abn = otab[2 * nsteps + tt];
            out = xs * sqrtf(abn) + sqrtf(1.f - abn) * eps;
        } else {
            const float ab = otab[tt], abp = otab[nsteps + tt];
            const float sigma = eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
            out = xs * sqrtf(abp) + sqrtf(1.f - abp - sigma * sigma) * eps;
            if (tt != 0) out += sigma * noise[i];
        }
    }
    sample[i] = out;
    if (xstart) xstart[i] = xs;
}

// The raw x0 prediction of p_mean_variance (:317-322), before process_xstart: what a denoised_fn hook is handed.
__global__ void obj_xstart_kernel(const float* __restrict__ mo, const float* __restrict__ x, const long* __restrict__ t,
                                  const float* __restrict__ tab, int nsteps, int mean_type, int var_type,
                                  float* __restrict__ xstart, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const long ostride = var_type == OBJ_LEARNED_RANGE ? 2 * (long)per : (long)per;
    const float m = mo[n * ostride + e];
    xstart[i] = mean_type == OBJ_START_X ? m : tab[2 * nsteps + tt] * x[i] - tab[3 * nsteps + tt] * m;
}

// obj_step_kernel with the sampler hooks of the reference folded in.  xstart_in (what denoised_fn returned) replaces the kernel's own
// x0 prediction and is clipped after it, as process_xstart does (:310-315).  cond_grad = cond_fn's gradient: p_sample applies
// condition_mean (:346-356: mean += variance x grad, pred_xstart unchanged, the noise added after it); the DDIM modes apply
// condition_score (:358-374: eps moved by -sqrt(1 - acp) x grad, x0 re-derived from it and NOT clipped again: x0 moves by
// sqrt_recipm1_acp x sqrt(1 - acp) x grad), and the DDIM update then re-derives eps from that x0 as the reference does.  `mean` receives the (conditioned) posterior mean; `sample` may be null
// when only pred_xstart / mean are wanted.  mo may be null when nothing is read from it (see mapdit_obj_step_guided).
__global__ void obj_step_guided_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ noise,
                                       const long* __restrict__ t, const float* __restrict__ tab, const float* __restrict__ otab,
                                       int nsteps, int mean_type, int var_type, int clip, int mode, float eta,
                                       const float* __restrict__ xstart_in, const float* __restrict__ cond_grad,
                                       float* __restrict__ sample, float* __restrict__ xstart, float* __restrict__ mean, long total,
                                       int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const bool learned = var_type == OBJ_LEARNED_RANGE;
    const long ostride = learned ? 2 * (long)per : (long)per;
    const float x_t = x[i];
    const ObjCoef c = obj_coef(tab, otab, nsteps, tt);
    float xs;
    if (xstart_in) {
        xs = xstart_in[i];
    } else {
        const float m = mo[n * ostride + e];
        xs = mean_type == OBJ_START_X ? m : c.ra * x_t - c.rm1 * m;
    }
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    float out = 0.f, mu;
    if (mode == OBJ_STEP_PSAMPLE) {
        mu = c.c1 * xs + c.c2 * x_t;
        const bool draw = noise && tt != 0;
        if (cond_grad || draw) {
            float dlv_dv;
            const float lv = obj_logvar(var_type, c, learned ? mo[n * ostride + per + e] : 0.f, &dlv_dv);
            // p_mean_variance's "variance" is exp(log-variance) except for FIXED_SMALL at t = 0: posterior_variance[0] = 0, while
            // its clipped log repeats entry 1 (:162-166, 302-305)
            if (cond_grad) mu += (var_type == OBJ_FIXED_SMALL && tt == 0 ? 0.f : expf(lv)) * cond_grad[i];
            out = draw ? expf(0.5f * lv) * noise[i] : 0.f;
        }
        out += mu;
    } else {
        // condition_score: eps = (ra x - x0) / rm1 - sqrt(1 - acp) grad, x0 = ra x - rm1 eps.  Written as the shift of x0 it amounts
        // to: the round trip through eps costs |ra x| / |x0| roundings (1e-5 of a clipped x0 at the last timestep), and a zero
        // gradient has to leave the unguided step as it is
        if (cond_grad) xs += c.rm1 * sqrtf(1.f - otab[tt]) * cond_grad[i];
        mu = c.c1 * xs + c.c2 * x_t;
        if (sample) {
            const float eps = (c.ra * x_t - xs) / c.rm1;          // _predict_eps_from_xstart
            if (mode == OBJ_STEP_DDIM_REVERSE) {
                const float abn = otab[2 * nsteps + tt];
                out = xs * sqrtf(abn) + sqrtf(1.f - abn) * eps;
            } else {
                const float ab = otab[tt], abp = otab[nsteps + tt];
                const float sigma = eta * sqrtf((1.f - abp) / (1.f - ab)) * sqrtf(1.f - ab / abp);
                out = xs * sqrtf(abp) + sqrtf(1.f - abp - sigma * sigma) * eps;
                if (tt != 0) out += sigma * noise[i];
            }
        }
    }
    if (sample) sample[i] = out;
    if (xstart) xstart[i] = xs;
    if (mean) mean[i] = mu;
}

// _vb_terms_bpd (:682-713) plus calc_bpd_loop's per-timestep MSEs (:829-842), one block per sample: vb (bits), xstart_mse and,
// given the noise, mse of the re-derived eps.  Outputs land at [n * ld + (col_from_t ? nsteps - 1 - t[n] : 0)]: calc_bpd_loop
// stacks its terms in loop order, t = T-1 first.
__global__ __launch_bounds__(256) void obj_vb_terms_kernel(const float* __restrict__ mo, const float* __restrict__ x0,
                                                         const float* __restrict__ xt, const float* __restrict__ noise,
                                                         const long* __restrict__ t, const float* __restrict__ tab,
                                                         const float* __restrict__ otab, int nsteps, int mean_type, int var_type,
                                                         int clip, float* __restrict__ vb, float* __restrict__ xstart_mse,
                                                         float* __restrict__ mse, float* __restrict__ xstart, int ld, int col_from_t,
                                                         int per) {
    const int n = blockIdx.x;
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, t[n], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const ObjCoef c = obj_coef(tab, otab, nsteps, tt);
    const bool learned = var_type == OBJ_LEARNED_RANGE;
    const size_t ostride = learned ? 2 * (size_t)per : (size_t)per;
    const bool first = tt == 0;
    float a_vb = 0.f, a_x = 0.f, a_e = 0.f;
    for (int e = threadIdx.x; e < per; e += 256) {
        const size_t im = (size_t)n * ostride + e, ix = (size_t)n * per + e;
        const float m = mo[im], x_0 = x0[ix], x_t = xt[ix];
        float dlv_dv, d_lv, d_mean;
        const float lv = obj_logvar(var_type, c, learned ? mo[im + per] : 0.f, &dlv_dv);
        float xs = mean_type == OBJ_START_X ? m : c.ra * x_t - c.rm1 * m;
        if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
        const float mean = c.c1 * xs + c.c2 * x_t;
        const float tmean = c.c1 * x_0 + c.c2 * x_t;
        a_vb += obj_vb_term(first, x_0, mean, lv, tmean, c.minlog, &d_lv, &d_mean);
        const float dx = xs - x_0;
        a_x += dx * dx;
        if (noise) {
            const float de = (c.ra * x_t - xs) / c.rm1 - noise[ix];
            a_e += de * de;
        }
        if (xstart) xstart[ix] = xs;
    }
    block_sum3(a_vb, a_x, a_e);
    if (threadIdx.x == 0) {
        const float inv_per = 1.f / (float)per;
        const size_t o = (size_t)n * ld + (col_from_t ? nsteps - 1 - tt : 0);
        vb[o] = a_vb * inv_per * INV_LN2;
        if (xstart_mse) xstart_mse[o] = a_x * inv_per;
        if (mse && noise) mse[o] = a_e * inv_per;
    }
}

// _prior_bpd (:789-803): KL(q(x_T | x_0) || N(0, I)) in bits per dim; with vb [N][nsteps] given, total = sum_t vb[n, t] + prior.
__global__ __launch_bounds__(256) void prior_bpd_kernel(const float* __restrict__ x0, const float* __restrict__ tab,
                                                      const float* __restrict__ otab, int nsteps, const float* __restrict__ vb,
                                                      float* __restrict__ prior, float* __restrict__ total, int per) {
    const int n = blockIdx.x;
    const float sa = tab[nsteps - 1], lv1 = otab[4 * nsteps + nsteps - 1];
    const float ev = expf(lv1);
    float a = 0.f, s = 0.f, unused = 0.f;
    for (int e = threadIdx.x; e < per; e += 256) {
        const float m = sa * x0[(size_t)n * per + e];
        a += 0.5f * (-1.f + 0.f - lv1 + ev + m * m);
    }
    if (vb)
        for (int k = threadIdx.x; k < nsteps; k += 256) s += vb[(size_t)n * nsteps + k];
    block_sum3(a, s, unused);
    if (threadIdx.x == 0) {
        const float p = a / (float)per * INV_LN2;
        prior[n] = p;
        if (vb && total) total[n] = s + p;
    }
}

// One step of the multistep DPM-Solver++ (Lu et al. 2022, Algorithm 2) in data-prediction form: D = the x0 prediction at timestep
// tau[step] (p_mean_variance's, or xstart_in; clipped on request), sample = c_x x + c_0 D + c_1 hist, hist <- D.  The three
// coefficients of row `step` of ctab are built on the host (mapdit.h); row 0 is (0, 1, 0): the last step returns the x0 prediction.
// sample may alias x and hist is read before it is written, each by the thread that owns the element: none of the three is
// __restrict__.
__global__ void dpm_step_kernel(const float* __restrict__ mo, const float* x, float* hist, const long* __restrict__ step,
                                const float* __restrict__ ctab, const long* __restrict__ tau, int K, const float* __restrict__ tab,
                                int nsteps, int mean_type, int var_type, int clip, const float* __restrict__ xstart_in, float* sample,
                                float* __restrict__ xstart, long total, int per) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long n = i / per, e = i % per;
    const long k = MAPDIT_CHECKED_INDEX(diffusion, step[n], K, MAPDIT_DEVERR_TIMESTEP);
    const long tt = MAPDIT_CHECKED_INDEX(diffusion, tau[k], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const float cx = ctab[3 * k], c0 = ctab[3 * k + 1], c1 = ctab[3 * k + 2];
    const float x_t = x[i];
    float d;
    if (xstart_in) {
        d = xstart_in[i];
    } else {
        const long ostride = var_type == OBJ_LEARNED_RANGE ? 2 * (long)per : (long)per;
        const float m = mo[n * ostride + e];
        d = mean_type == OBJ_START_X ? m : tab[2 * nsteps + tt] * x_t - tab[3 * nsteps + tt] * m;
    }
    if (clip) d = fminf(fmaxf(d, -1.f), 1.f);
    const float prev = hist[i];
    sample[i] = cx * x_t + c0 * d + c1 * prev;
    hist[i] = d;
    if (xstart) xstart[i] = d;
}

bool obj_types_ok(int mean_type, int var_type) {
    return (mean_type == OBJ_EPSILON || mean_type == OBJ_START_X) && var_type >= OBJ_LEARNED_RANGE && var_type <= OBJ_FIXED_LARGE;
}

}  // namespace

extern "C" int mapdit_dpm_step(const float* model_out, const float* x, float* hist, const int64_t* step, const float* ctab,
                               const int64_t* tau, int K, const float* tab, int nsteps, int mean_type, int var_type, int clip_denoised,
                               const float* xstart_in, float* sample, float* pred_xstart, int N, int per_sample, void* stream) {
    MD_CHECK(x && hist && step && ctab && tau && tab && sample && N > 0 && per_sample > 0 && nsteps > 0 && K > 0,
             "dpm_step: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type), "dpm_step: bad objective");
    MD_CHECK(model_out || xstart_in, "dpm_step: this step reads the model output (null)");
    MD_CHECK(hist != x && hist != sample && hist != xstart_in && sample != xstart_in &&
                 (!pred_xstart || (pred_xstart != sample && pred_xstart != hist && pred_xstart != x && pred_xstart != xstart_in)),
             "dpm_step: overlapping arguments (only sample may alias x)");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(dpm_step_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, hist, (const long*)step,
                       ctab, (const long*)tau, K, tab, nsteps, mean_type, var_type, clip_denoised, xstart_in, sample, pred_xstart, total,
                       per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_loss_fwd(const float* model_out, const float* x0, const float* xt, const float* noise, const int64_t* t,
                                   const float* tab, const float* otab, int nsteps, int mean_type, int var_type, int loss_type,
                                   float* mse, float* vb, float* loss, float* G, int N, int per_sample, void* stream) {
    MD_CHECK(model_out && x0 && xt && t && tab && otab && loss && G && N > 0 && per_sample > 0 && nsteps > 0,
             "obj_loss_fwd: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type) && loss_type >= OBJ_MSE && loss_type <= OBJ_RESCALED_KL, "obj_loss_fwd: bad objective");
    const bool is_kl = loss_type >= OBJ_KL;
    MD_CHECK(is_kl || (mse && (mean_type == OBJ_START_X || noise)), "obj_loss_fwd: the MSE losses need mse (and noise for EPSILON)");
    MD_CHECK(is_kl || var_type != OBJ_LEARNED_RANGE || vb, "obj_loss_fwd: LEARNED_RANGE with an MSE loss needs vb");
    hipLaunchKernelGGL(obj_loss_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, model_out, x0, xt, noise, (const long*)t, tab, otab,
                       nsteps, mean_type, var_type, loss_type, mse, vb, loss, G, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_loss_bwd(const float* G, const float* g_loss, const float* g_mse, const float* g_vb, float* dout, int N,
                                   int per_sample, int groups, void* stream) {
    MD_CHECK(G && dout && N > 0 && per_sample > 0 && (groups == 1 || groups == 2), "obj_loss_bwd: null/empty argument");
    const long total = (long)N * groups * per_sample;
    hipLaunchKernelGGL(obj_loss_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, G, g_loss, g_mse, g_vb, dout,
                       total, per_sample, groups);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_step(const float* model_out, const float* x, const float* noise, const int64_t* t, const float* tab,
                               const float* otab, int nsteps, int mean_type, int var_type, int clip_denoised, int mode, float eta,
                               float* sample, float* pred_xstart, int N, int per_sample, void* stream) {
    MD_CHECK(model_out && x && t && tab && otab && sample && N > 0 && per_sample > 0 && nsteps > 0, "obj_step: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type) && mode >= OBJ_STEP_PSAMPLE && mode <= OBJ_STEP_DDIM_REVERSE, "obj_step: bad objective/mode");
    MD_CHECK(mode != OBJ_STEP_DDIM || noise, "obj_step: the DDIM step needs the noise tensor");
    MD_CHECK(mode != OBJ_STEP_DDIM_REVERSE || eta == 0.f, "obj_step: the reverse ODE is deterministic (eta must be 0)");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(obj_step_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, noise, (const long*)t,
                       tab, otab, nsteps, mean_type, var_type, clip_denoised, mode, eta, sample, pred_xstart, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_xstart(const float* model_out, const float* x, const int64_t* t, const float* tab, int nsteps, int mean_type,
                                 int var_type, float* xstart, int N, int per_sample, void* stream) {
    MD_CHECK(model_out && x && t && tab && xstart && N > 0 && per_sample > 0 && nsteps > 0, "obj_xstart: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type), "obj_xstart: bad objective");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(obj_xstart_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, (const long*)t, tab,
                       nsteps, mean_type, var_type, xstart, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_step_guided(const float* model_out, const float* x, const float* noise, const int64_t* t, const float* tab,
                                      const float* otab, int nsteps, int mean_type, int var_type, int clip_denoised, int mode,
                                      float eta, const float* xstart_in, const float* cond_grad, float* sample, float* pred_xstart,
                                      float* mean, int N, int per_sample, void* stream) {
    MD_CHECK(x && t && tab && otab && (sample || pred_xstart || mean) && N > 0 && per_sample > 0 && nsteps > 0,
             "obj_step_guided: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type) && mode >= OBJ_STEP_PSAMPLE && mode <= OBJ_STEP_DDIM_REVERSE,
             "obj_step_guided: bad objective/mode");
    // the model output is read for the x0 prediction (no xstart_in) and for the learned variance of a p_sample step
    const bool reads_var = mode == OBJ_STEP_PSAMPLE && var_type == OBJ_LEARNED_RANGE && (cond_grad || noise);
    MD_CHECK(model_out || (xstart_in && !reads_var), "obj_step_guided: this step reads the model output (null)");
    MD_CHECK(mode != OBJ_STEP_DDIM || noise || !sample, "obj_step_guided: the DDIM step needs the noise tensor");
    MD_CHECK(mode != OBJ_STEP_DDIM_REVERSE || eta == 0.f, "obj_step_guided: the reverse ODE is deterministic (eta must be 0)");
    const long total = (long)N * per_sample;
    hipLaunchKernelGGL(obj_step_guided_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, model_out, x, noise,
                       (const long*)t, tab, otab, nsteps, mean_type, var_type, clip_denoised, mode, eta, xstart_in, cond_grad, sample,
                       pred_xstart, mean, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_obj_vb_terms(const float* model_out, const float* x0, const float* xt, const float* noise, const int64_t* t,
                                   const float* tab, const float* otab, int nsteps, int mean_type, int var_type, int clip_denoised,
                                   float* vb, float* xstart_mse, float* mse, float* pred_xstart, int ld, int col_from_t, int N,
                                   int per_sample, void* stream) {
    MD_CHECK(model_out && x0 && xt && t && tab && otab && vb && N > 0 && per_sample > 0 && nsteps > 0, "obj_vb_terms: null/empty argument");
    MD_CHECK(obj_types_ok(mean_type, var_type), "obj_vb_terms: bad objective");
    MD_CHECK(col_from_t ? ld >= nsteps : ld >= 1, "obj_vb_terms: ld must hold a column per timestep");
    hipLaunchKernelGGL(obj_vb_terms_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, model_out, x0, xt, noise, (const long*)t, tab,
                       otab, nsteps, mean_type, var_type, clip_denoised, vb, xstart_mse, mse, pred_xstart, ld, col_from_t, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_prior_bpd(const float* x0, const float* tab, const float* otab, int nsteps, const float* vb, float* prior,
                                float* total, int N, int per_sample, void* stream) {
    MD_CHECK(x0 && tab && otab && prior && N > 0 && per_sample > 0 && nsteps > 0, "prior_bpd: null/empty argument");
    MD_CHECK(!vb || total, "prior_bpd: vb given without total");
    hipLaunchKernelGGL(prior_bpd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, x0, tab, otab, nsteps, vb, prior, total, per_sample);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
