// Counter-based draws of the samplers (sample_rng.py, --sample-rng counter): the initial latent, the label and the noise of every
// reverse step of sample s as a pure function of (seed, s) - mapdit.h, "Counter-based sampler draws", is the contract.  The generator
// and the fp32 normal recipe are dataset.hip's (philox.h); the tags in counter word c3 keep the families' counters apart.
//
// The fused steps (mapdit_psample_step_counter, mapdit_obj_step_counter) generate a step's noise in registers and must give the bits
// of diffusion.hip's p_sample_kernel / obj_step_kernel fed with mapdit_sample_noise's tensor.  Those kernels are built with
// -ffp-contract=fast, under which the compiler chooses which products fuse into which sums - inside the inlined library expf too;
// psample_elem / obj_step_elem / exp_as_diffusion below write that choice down operation by operation under `#pragma clang fp
// contract(off)` (this file is built with fast-honor-pragmas, which obeys it), read off those kernels' device code, so nothing here is
// left to a heuristic and diffusion.hip is untouched.  tests/test_sample_rng_gpu.py holds the two families together bit for bit.
#include "common.h"
#include "philox.h"

MAPDIT_DEFINE_DEV_ERROR(samplerng)

namespace {

#define SMP_LANES 256

enum { OBJ_EPSILON = 0, OBJ_START_X = 1 };
enum { OBJ_LEARNED_RANGE = 0, OBJ_FIXED_SMALL = 1, OBJ_FIXED_LARGE = 2 };
enum { OBJ_STEP_PSAMPLE = 0, OBJ_STEP_DDIM = 1, OBJ_STEP_DDIM_REVERSE = 2 };

// Workgroup b: row j = b / chunks, the groups of four elements (b % chunks) * 256 + lane of that row (uniform per workgroup).  The first
// N lanes of the grid also write the label of row = their lane number.  vec: per % 4 == 0 and the plane is 16-byte aligned.
__global__ __launch_bounds__(SMP_LANES) void sample_draw_kernel(uint32_t k0, uint32_t k1, const long* __restrict__ index, int N, long per,
                                                                uint32_t chunks, uint32_t num_classes, float* __restrict__ z, int vec,
                                                                long* __restrict__ y) {
    const long lane = (long)blockIdx.x * SMP_LANES + threadIdx.x;
    if (y && lane < N) {
        const u32x4 a = philox4x32_10(0u, (uint32_t)index[lane], 0u, MAPDIT_TAG_SMPY, k0, k1);
        y[lane] = (long)(((uint64_t)a.x * num_classes) >> 32);
    }
    if (!z) return;
    const uint32_t j = blockIdx.x / chunks;                            // < N: the grid is N * chunks workgroups
    const long g = (long)(blockIdx.x - j * chunks) * SMP_LANES + threadIdx.x;
    const long i0 = 4 * g;
    if (i0 >= per) return;
    const long at = (long)j * per + i0;
    float v[4];
    philox_normal4((uint32_t)g, (uint32_t)index[j], 0u, MAPDIT_TAG_SMPZ, k0, k1, v);
    if (vec) {
        *reinterpret_cast<float4*>(z + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (i0 + l < per) z[at + l] = v[l];
    }
}

__global__ __launch_bounds__(SMP_LANES) void sample_noise_kernel(uint32_t k0, uint32_t k1, const long* __restrict__ index,
                                                                 const long* __restrict__ t, long per, uint32_t chunks,
                                                                 float* __restrict__ noise, int vec) {
    const uint32_t j = blockIdx.x / chunks;
    const long g = (long)(blockIdx.x - j * chunks) * SMP_LANES + threadIdx.x;
    const long i0 = 4 * g;
    if (i0 >= per) return;
    const long at = (long)j * per + i0;
    float v[4];
    philox_normal4((uint32_t)g, (uint32_t)index[j], (uint32_t)t[j], MAPDIT_TAG_SMPN, k0, k1, v);
    if (vec) {
        *reinterpret_cast<float4*>(noise + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (i0 + l < per) noise[at + l] = v[l];
    }
}

// expf as diffusion.hip's kernels compute it.  That file is built with -ffp-contract=fast, which also fuses inside the device library's
// expf once it is inlined: the reduced argument ph - rint(ph), ph = fl(x log2 e), exact as the library writes it, becomes ONE fused
// x log2 e - rint(ph) there.  Under fast-honor-pragmas the library's own form comes out, a last-bit difference in some results; the
// fused steps owe diffusion.hip's bits, so its sequence is written down: hi / lo split of x log2 e, the hardware's 2^a, the scaling by
// 2^rint(ph), and the library's underflow / overflow limits.
__device__ __forceinline__ float exp_as_diffusion(float x) {
#pragma clang fp contract(off)
    const float log2e_hi = 0x1.715476p+0f, log2e_lo = 0x1.4ae0bep-26f;                  // 0x3fb8aa3b, 0x32a5705f
    const float ph = x * log2e_hi;
    float pl = __builtin_fmaf(x, log2e_hi, -ph);
    pl = __builtin_fmaf(x, log2e_lo, pl);
    const float e = __builtin_rintf(ph);
    const float a = __builtin_fmaf(x, log2e_hi, -e) + pl;
    float r = __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a), (int)e);
    r = x < -0x1.9d1dap+6f ? 0.f : r;                                                    // 0xc2ce8ed0
    return x > 0x1.62e43p+6f ? __builtin_inff() : r;                                     // 0x42b17218
}

struct StepCoef {
    float ra, rm1, minlog, maxlog, c1, c2, fixlog, ab, abp;
};

// frac maxlog + (1 - frac) minlog, frac = (v + 1) / 2, as p_sample_kernel and obj_logvar compile: 1 - frac is ONE fused operation on v + 1
__device__ __forceinline__ float learned_logvar(float v, float minlog, float maxlog) {
#pragma clang fp contract(off)
    const float a = v + 1.f;
    const float frac = a * 0.5f;
    const float omf = __builtin_fmaf(a, -0.5f, 1.f);
    return __builtin_fmaf(maxlog, frac, minlog * omf);
}

// One element of p_sample_kernel (diffusion.hip): x0^ and the posterior mean fused as there, the noise term rounded on its own and
// then added (there the product sits behind the `tt != 0` branch, in another basic block than the sum).
__device__ __forceinline__ float psample_elem(const StepCoef& c, float eps, float v, float x_t, int clip, bool first, float nz, float* xs_out) {
#pragma clang fp contract(off)
    const float lv = learned_logvar(v, c.minlog, c.maxlog);
    float xs = __builtin_fmaf(c.ra, x_t, -(c.rm1 * eps));
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    const float mean = __builtin_fmaf(x_t, c.c2, c.c1 * xs);
    *xs_out = xs;
    return mean + (first ? 0.f : exp_as_diffusion(0.5f * lv) * nz);
}

// One element of obj_step_kernel (diffusion.hip), modes p_sample and DDIM: ra x_t is rounded once and shared by x0^ and the re-derived
// noise; the noise term is fused into the sum in both modes.
__device__ __forceinline__ float obj_step_elem(const StepCoef& c, int mean_type, int var_type, int clip, int mode, float eta, float m,
                                               float v, float x_t, bool first, float nz, float* xs_out) {
#pragma clang fp contract(off)
    const float p = c.ra * x_t;
    float xs = mean_type == OBJ_START_X ? m : __builtin_fmaf(-c.rm1, m, p);
    if (clip) xs = fminf(fmaxf(xs, -1.f), 1.f);
    *xs_out = xs;
    float out;
    if (mode == OBJ_STEP_PSAMPLE) {
        out = __builtin_fmaf(x_t, c.c2, c.c1 * xs);
        if (!first) {
            const float lv = var_type == OBJ_LEARNED_RANGE ? learned_logvar(v, c.minlog, c.maxlog)
                                                           : var_type == OBJ_FIXED_SMALL ? c.minlog : c.fixlog;
            out = __builtin_fmaf(exp_as_diffusion(0.5f * lv), nz, out);
        }
    } else {
        const float eps = (p - xs) / c.rm1;                            // _predict_eps_from_xstart
        const float sigma = eta * sqrtf((1.f - c.abp) / (1.f - c.ab)) * sqrtf(1.f - c.ab / c.abp);
        out = __builtin_fmaf(xs, sqrtf(c.abp), sqrtf(__builtin_fmaf(-sigma, sigma, 1.f - c.abp)) * eps);
        if (!first) out = __builtin_fmaf(sigma, nz, out);
    }
    return out;
}

struct StepArgs {
    const float* mo;
    const float* x;                  // (no __restrict__ on x / sample: sample may be x itself)
    const long* index;
    const long* t;
    const float* tab;
    const float* otab;               // null: the default objective's math (p_sample_kernel)
    float* sample;
    float* xstart;
    uint32_t k0, k1, chunks;
    int nsteps, mean_type, var_type, clip, mode, vec;
    float eta;
    long per;
};

// One lane: one Philox call = the four normals of elements 4g .. 4g + 3 of row j, the four x, mean-channel and variance-channel values
// of those elements, four results.  Everything a lane reads is read before it writes, and no two lanes share an element.
template <bool OBJ>
__global__ __launch_bounds__(SMP_LANES) void sample_step_kernel(StepArgs a) {
    const uint32_t j = blockIdx.x / a.chunks;
    const long g = (long)(blockIdx.x - j * a.chunks) * SMP_LANES + threadIdx.x;
    const long i0 = 4 * g, per = a.per;
    if (i0 >= per) return;
    const int nsteps = a.nsteps;
    const long tt = MAPDIT_CHECKED_INDEX(samplerng, a.t[j], nsteps, MAPDIT_DEVERR_TIMESTEP);
    const bool learned = !OBJ || a.var_type == OBJ_LEARNED_RANGE;
    const long at = (long)j * per + i0;
    const float* mrow = a.mo + (long)j * (learned ? 2 * per : per) + i0;
    float m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f}, xt[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.vec) {
        const float4 m4 = *reinterpret_cast<const float4*>(mrow), x4 = *reinterpret_cast<const float4*>(a.x + at);
        m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
        xt[0] = x4.x; xt[1] = x4.y; xt[2] = x4.z; xt[3] = x4.w;
        if (learned) {
            const float4 v4 = *reinterpret_cast<const float4*>(mrow + per);
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
        }
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (i0 + l < per) {
                m[l] = mrow[l];
                xt[l] = a.x[at + l];
                if (learned) v[l] = mrow[per + l];
            }
    }
    StepCoef c;
    c.ra = a.tab[2 * nsteps + tt]; c.rm1 = a.tab[3 * nsteps + tt]; c.minlog = a.tab[4 * nsteps + tt]; c.maxlog = a.tab[5 * nsteps + tt];
    c.c1 = a.tab[6 * nsteps + tt]; c.c2 = a.tab[7 * nsteps + tt];
    c.fixlog = c.ab = c.abp = 0.f;
    if (OBJ) {
        c.ab = a.otab[tt]; c.abp = a.otab[nsteps + tt]; c.fixlog = a.otab[3 * nsteps + tt];
    }
    const bool first = tt == 0;                                        // the step at t = 0 adds no noise: no draw (uniform per workgroup)
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (!first) philox_normal4((uint32_t)g, (uint32_t)a.index[j], (uint32_t)tt, MAPDIT_TAG_SMPN, a.k0, a.k1, nz);
    float out[4], xs[4];
#pragma unroll
    for (int l = 0; l < 4; ++l)
        out[l] = OBJ ? obj_step_elem(c, a.mean_type, a.var_type, a.clip, a.mode, a.eta, m[l], v[l], xt[l], first, nz[l], &xs[l])
                     : psample_elem(c, m[l], v[l], xt[l], a.clip, first, nz[l], &xs[l]);
    if (a.vec) {
        *reinterpret_cast<float4*>(a.sample + at) = make_float4(out[0], out[1], out[2], out[3]);
        if (a.xstart) *reinterpret_cast<float4*>(a.xstart + at) = make_float4(xs[0], xs[1], xs[2], xs[3]);
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (i0 + l < per) {
                a.sample[at + l] = out[l];
                if (a.xstart) a.xstart[at + l] = xs[l];
            }
    }
}

// rows * chunks workgroups, chunks = ceil(ceil(per / 4) / 256); 0 where they do not fit a grid
long plane_chunks(int N, long per, long* blocks) {
    const long groups = (per + 3) / 4;
    const long chunks = (groups + SMP_LANES - 1) / SMP_LANES;
    *blocks = (long)N * chunks;
    return chunks;
}

int launch_step(const char* who, StepArgs a, uint64_t seed, int N, int per_sample, void* stream) {
    long blocks;
    a.chunks = (uint32_t)plane_chunks(N, per_sample, &blocks);
    MD_CHECK(blocks <= 0x7fffffffL, "%s: N=%d rows of per_sample=%d elements need %ld workgroups (at most 2^31 - 1)", who, N, per_sample, blocks);
    MD_CHECK(aligned(a.mo, 4) && aligned(a.x, 4) && aligned(a.sample, 4) && aligned(a.xstart, 4) && aligned(a.index, 8) && aligned(a.t, 8),
             "%s: unaligned pointer", who);
    MD_CHECK(a.sample != a.xstart && a.xstart != a.x, "%s: pred_xstart overlaps sample or x (only sample may be x itself)", who);
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.per = per_sample;
    a.vec = per_sample % 4 == 0 && aligned(a.mo, 16) && aligned(a.x, 16) && aligned(a.sample, 16) && aligned(a.xstart, 16) ? 1 : 0;
    if (a.otab)
        hipLaunchKernelGGL(sample_step_kernel<true>, dim3((unsigned)blocks), dim3(SMP_LANES), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sample_step_kernel<false>, dim3((unsigned)blocks), dim3(SMP_LANES), 0, (hipStream_t)stream, a);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

}  // namespace

extern "C" int mapdit_sample_draw(uint64_t seed, const int64_t* index, int N, long per, int num_classes, float* z, int64_t* y, void* stream) {
    MD_CHECK(index && N >= 1 && per >= 1, "sample_draw: N=%d rows of per=%ld elements (both >= 1) and their index array", N, per);
    MD_CHECK(per <= (1L << 34) / N, "sample_draw: N * per = %d * %ld values exceed 2^34", N, per);
    MD_CHECK(!y || num_classes >= 1, "sample_draw: num_classes=%d (>= 1 where y is asked for)", num_classes);
    MD_CHECK(aligned(index, 8) && aligned(z, 4) && aligned(y, 8), "sample_draw: unaligned pointer");
    if (!z && !y) return MAPDIT_OK;
    long blocks;
    long chunks = plane_chunks(N, per, &blocks);
    if (!z) {
        chunks = 1;
        blocks = ((long)N + SMP_LANES - 1) / SMP_LANES;
    }
    MD_CHECK(blocks <= 0x7fffffffL, "sample_draw: N=%d rows of per=%ld elements need %ld workgroups (at most 2^31 - 1)", N, per, blocks);
    hipLaunchKernelGGL(sample_draw_kernel, dim3((unsigned)blocks), dim3(SMP_LANES), 0, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (const long*)index, N, per, (uint32_t)chunks, (uint32_t)(y ? num_classes : 1), z,
                       per % 4 == 0 && aligned(z, 16) ? 1 : 0, (long*)y);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_sample_noise(uint64_t seed, const int64_t* index, const int64_t* t, int N, long per, float* noise, void* stream) {
    MD_CHECK(index && t && noise && N >= 1 && per >= 1, "sample_noise: null/empty argument (N=%d, per=%ld)", N, per);
    MD_CHECK(per <= (1L << 34) / N, "sample_noise: N * per = %d * %ld values exceed 2^34", N, per);
    MD_CHECK(aligned(index, 8) && aligned(t, 8) && aligned(noise, 4), "sample_noise: unaligned pointer");
    long blocks;
    const long chunks = plane_chunks(N, per, &blocks);
    MD_CHECK(blocks <= 0x7fffffffL, "sample_noise: N=%d rows of per=%ld elements need %ld workgroups (at most 2^31 - 1)", N, per, blocks);
    hipLaunchKernelGGL(sample_noise_kernel, dim3((unsigned)blocks), dim3(SMP_LANES), 0, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (const long*)index, (const long*)t, per, (uint32_t)chunks, noise,
                       per % 4 == 0 && aligned(noise, 16) ? 1 : 0);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_psample_step_counter(const float* model_out, const float* x, uint64_t seed, const int64_t* index, const int64_t* t,
                                           const float* tab, int nsteps, int clip_denoised, float* sample, float* pred_xstart, int N,
                                           int per_sample, void* stream) {
    MD_CHECK(model_out && x && index && t && tab && sample && N > 0 && per_sample > 0 && nsteps > 0, "psample_step_counter: null/empty argument");
    StepArgs a = {};
    a.mo = model_out; a.x = x; a.index = (const long*)index; a.t = (const long*)t; a.tab = tab; a.otab = nullptr;
    a.sample = sample; a.xstart = pred_xstart; a.nsteps = nsteps; a.clip = clip_denoised;
    return launch_step("psample_step_counter", a, seed, N, per_sample, stream);
}

extern "C" int mapdit_obj_step_counter(const float* model_out, const float* x, uint64_t seed, const int64_t* index, const int64_t* t,
                                       const float* tab, const float* otab, int nsteps, int mean_type, int var_type, int clip_denoised,
                                       int mode, float eta, float* sample, float* pred_xstart, int N, int per_sample, void* stream) {
    MD_CHECK(model_out && x && index && t && tab && otab && sample && N > 0 && per_sample > 0 && nsteps > 0,
             "obj_step_counter: null/empty argument");
    MD_CHECK((mean_type == OBJ_EPSILON || mean_type == OBJ_START_X) && var_type >= OBJ_LEARNED_RANGE && var_type <= OBJ_FIXED_LARGE,
             "obj_step_counter: bad objective");
    MD_CHECK(mode != OBJ_STEP_DDIM_REVERSE, "obj_step_counter: the reverse ODE (mode 2) draws no noise: use mapdit_obj_step");
    MD_CHECK(mode == OBJ_STEP_PSAMPLE || mode == OBJ_STEP_DDIM, "obj_step_counter: bad mode %d (0 p_sample, 1 DDIM)", mode);
    MD_CHECK(mode != OBJ_STEP_DDIM || eta >= 0.f, "obj_step_counter: eta=%g (>= 0)", (double)eta);
    StepArgs a = {};
    a.mo = model_out; a.x = x; a.index = (const long*)index; a.t = (const long*)t; a.tab = tab; a.otab = otab;
    a.sample = sample; a.xstart = pred_xstart; a.nsteps = nsteps; a.mean_type = mean_type; a.var_type = var_type; a.clip = clip_denoised;
    a.mode = mode; a.eta = eta;
    return launch_step("obj_step_counter", a, seed, N, per_sample, stream);
}
