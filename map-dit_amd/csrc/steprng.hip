// Counter-based draws of a training step (train.py --step-rng counter, step_rng.py): diffusion / flow noise, timesteps, the uniforms and
// normals the other timestep samplers map, label drops and the --synthetic batch, in ONE launch and as a pure function of
// (seed, optimiser step, slot in the global batch) - mapdit.h, "Counter-based step draws", is the contract.  The generator and the fp32
// normal recipe are dataset.hip's (philox.h); the tags in counter word c3 keep the two files' counters apart.
#include "common.h"
#include "philox.h"

namespace {

#define SR_LANES 256

// Workgroup b: row j = b / chunks of the planes, the groups of four elements (b % chunks) * 256 + lane of that row (both uniform per
// workgroup: the division is scalar).  The first `count` lanes of the grid also write the per-slot scalars of slot = their lane number;
// the grid holds count * chunks * 256 >= count lanes.  vec_*: per % 4 == 0 and the plane is 16-byte aligned - every group is whole and
// every group's address a multiple of 16.
__global__ __launch_bounds__(SR_LANES) void step_draw_kernel(uint32_t k0, uint32_t k1, uint32_t step, uint32_t first, int count, long per,
                                                             uint32_t chunks, uint32_t T, uint32_t num_classes, uint32_t thr,
                                                             float* __restrict__ eps, int vec_eps, float* __restrict__ x_syn, int vec_syn,
                                                             long* __restrict__ t, double* __restrict__ u, double* __restrict__ z,
                                                             long* __restrict__ drop, long* __restrict__ y_syn) {
    const long lane = (long)blockIdx.x * SR_LANES + threadIdx.x;
    if (lane < count && (t || u || z || drop || y_syn)) {
        const uint32_t slot = first + (uint32_t)lane;                  // first + count <= 2^32: checked by the caller
        if (t || u || drop) {
            const u32x4 a = philox4x32_10(0u, slot, step, MAPDIT_TAG_STEP, k0, k1);
            if (t) t[lane] = (long)(((uint64_t)a.x * T) >> 32);
            if (drop) drop[lane] = (a.y >> 8) < thr ? 1 : 0;
            if (u) u[lane] = (double)(((uint64_t)a.z << 21) | (uint64_t)(a.w >> 11)) * 0x1p-53;      // 53 bits: the conversion is exact
        }
        if (y_syn || z) {
            const u32x4 b = philox4x32_10(1u, slot, step, MAPDIT_TAG_STEP, k0, k1);
            if (y_syn) y_syn[lane] = (long)(((uint64_t)b.x * num_classes) >> 32);
            if (z) {
                float zc, zs;
                box_muller(b.z, b.w, &zc, &zs);
                z[lane] = (double)zc;
            }
        }
    }
    if (!eps && !x_syn) return;
    const uint32_t j = blockIdx.x / chunks;                            // < count: the grid is count * chunks workgroups
    const long g = (long)(blockIdx.x - j * chunks) * SR_LANES + threadIdx.x;
    const long i0 = 4 * g;
    if (i0 >= per) return;
    const long at = (long)j * per + i0;
    const uint32_t slot = first + j;
    float v[4];
    if (eps) {
        philox_normal4((uint32_t)g, slot, step, MAPDIT_TAG_EPS, k0, k1, v);
        if (vec_eps) {
            *reinterpret_cast<float4*>(eps + at) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (i0 + l < per) eps[at + l] = v[l];
        }
    }
    if (x_syn) {
        philox_normal4((uint32_t)g, slot, step, MAPDIT_TAG_SYNX, k0, k1, v);
        if (vec_syn) {
            *reinterpret_cast<float4*>(x_syn + at) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (i0 + l < per) x_syn[at + l] = v[l];
        }
    }
}

}  // namespace

// thr of the label drop: the smallest integer k with k 2^-24 >= (float)drop_prob, so that (w >> 8) < thr is (w >> 8) 2^-24 < p for the
// fp32 p the reference compares with (label_embedder.py:23: torch.rand(n) < p; torch's fp32 uniform is a 24-bit integer times 2^-24).
static uint32_t drop_threshold(float drop_prob) {
    const double x = (double)drop_prob * 16777216.0;                   // exact: an fp32 value times a power of two
    const uint32_t k = (uint32_t)x;
    return (double)k < x ? k + 1 : k;
}

extern "C" int mapdit_step_draw(uint64_t seed, uint32_t step, long first_slot, int count, long per, int T, int num_classes, float drop_prob,
                                float* eps, float* x_syn, int64_t* t, double* u, double* z, int64_t* drop, int64_t* y_syn, void* stream) {
    MD_CHECK(count >= 1 && per >= 1, "step_draw: count=%d slots of per=%ld elements (both >= 1)", count, per);
    MD_CHECK(first_slot >= 0 && first_slot <= (1L << 32) - count,
             "step_draw: slots [%ld, %ld + %d) do not lie in [0, 2^32): the slot is a 32-bit counter word", first_slot, first_slot, count);
    MD_CHECK(per <= (1L << 34) / count, "step_draw: count * per = %d * %ld values exceed 2^34", count, per);
    MD_CHECK(!t || T >= 1, "step_draw: T=%d timesteps (1 <= T <= 2^31)", T);
    MD_CHECK(!y_syn || num_classes >= 1, "step_draw: num_classes=%d (>= 1 where y_syn is asked for)", num_classes);
    MD_CHECK(!drop || (drop_prob >= 0.f && drop_prob <= 1.f), "step_draw: drop_prob=%g does not lie in [0, 1]", (double)drop_prob);
    MD_CHECK(aligned(eps, 4) && aligned(x_syn, 4) && aligned(t, 8) && aligned(u, 8) && aligned(z, 8) && aligned(drop, 8) && aligned(y_syn, 8),
             "step_draw: unaligned pointer");
    if (!eps && !x_syn && !t && !u && !z && !drop && !y_syn) return MAPDIT_OK;
    const bool planes = eps || x_syn;
    const long groups = (per + 3) / 4;
    const long chunks = planes ? (groups + SR_LANES - 1) / SR_LANES : 1;               // <= 2^24
    const long blocks = planes ? (long)count * chunks : ((long)count + SR_LANES - 1) / SR_LANES;
    MD_CHECK(blocks <= 0x7fffffffL, "step_draw: count=%d rows of per=%ld elements need %ld workgroups (at most 2^31 - 1)", count, per, blocks);
    hipLaunchKernelGGL(step_draw_kernel, dim3((unsigned)blocks), dim3(SR_LANES), 0, (hipStream_t)stream, (uint32_t)seed, (uint32_t)(seed >> 32),
                       step, (uint32_t)first_slot, count, per, (uint32_t)chunks, (uint32_t)(t ? T : 1), (uint32_t)(y_syn ? num_classes : 1),
                       drop ? drop_threshold(drop_prob) : 0u, eps, per % 4 == 0 && aligned(eps, 16) ? 1 : 0, x_syn,
                       per % 4 == 0 && aligned(x_syn, 16) ? 1 : 0, (long*)t, u, z, (long*)drop, (long*)y_syn);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
