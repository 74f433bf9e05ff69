// Device-resident latent data set (train.py --data-loader device, data.py): the epoch shuffle, the gather of a batch and the draw from
// each sample's posterior, in one launch and as a pure function of (seed, epoch, position) - mapdit.h, "Device-resident latent data set",
// is the contract.  The generator (Philox4x32-10) and the fp32 normal recipe live in philox.h, which steprng.hip shares: they exist once.
#include <math.h>

#include "common.h"
#include "philox.h"

// mean + eps * std is two roundings and (f - m) / s a correctly rounded subtraction and division in the reference's torch ops
// (train.py:170-176): no fused multiply-add here.  -ffp-contract=fast disregards the pragma (the backend fuses whatever it meets,
// __fmul_rn / __fadd_rn included), so the Makefile builds this file with -ffp-contract=fast-honor-pragmas.
#pragma clang fp contract(off)

namespace {

#define DS_TAG_PERM 0x5045524Du    // "PERM"
#define DS_TAG_NOISE 0x4E4F4953u   // "NOIS"
#define DS_LANES 256
#define DS_MAX_CHUNKS 64           // workgroups per sample at most; the groups of four elements beyond them are strided over

// The epoch permutation of [0, N): a balanced Feistel network of four rounds over [0, 2^(2 half)), walked until the value is below N.
// 2^(2 half) <= 4 N, so a walk takes fewer than four turns on average; it ends because the network is a bijection (the walk from a
// value below N returns to a value below N).
__device__ __forceinline__ uint32_t feistel_perm(uint32_t x, uint32_t N, int half, uint32_t epoch, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << half) - 1u;
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t f = philox4x32_10(R, r, epoch, DS_TAG_PERM, k0, k1).x & mask;
            const uint32_t t = L ^ f;
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= N);
    return x;
}

__global__ __launch_bounds__(DS_LANES) void philox_normal_kernel(uint32_t k0, uint32_t k1, uint32_t c1, uint32_t c2, uint32_t c3,
                                                                 float* __restrict__ out, long n, int vec) {
    const long g = (long)blockIdx.x * DS_LANES + threadIdx.x;          // the group of four: elements 4 g .. 4 g + 3
    if (4 * g >= n) return;
    float z[4];
    philox_normal4((uint32_t)g, c1, c2, c3, k0, k1, z);
    if (vec && 4 * g + 4 <= n) {
        *reinterpret_cast<float4*>(out + 4 * g) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (4 * g + l < n) out[4 * g + l] = z[l];
    }
}

__global__ __launch_bounds__(DS_LANES) void data_perm_kernel(uint32_t k0, uint32_t k1, uint32_t epoch, uint32_t N, int half, long first, long count,
                                                             long* __restrict__ idx) {
    const long j = (long)blockIdx.x * DS_LANES + threadIdx.x;
    if (j >= count) return;
    idx[j] = (long)feistel_perm((uint32_t)(first + j), N, half, epoch, k0, k1);
}

// Workgroup (j, chunk): sample j of the batch, the groups of four elements chunk * 256 + lane + m * chunks * 256 of its row.  Lane 0
// walks the permutation once for the workgroup.  VEC: every row of means / stds / x (and eps_in) starts on a 16-byte boundary and
// holds whole groups - 16 bytes per lane and access; otherwise element by element, the last group of a row cut short.
template <bool VEC>
__global__ __launch_bounds__(DS_LANES) void data_batch_kernel(const float* __restrict__ means, const float* __restrict__ stds,
                                                              const long* __restrict__ labels, uint32_t N, int half, int hw, int per_sample,
                                                              const float* __restrict__ ch_mean, const float* __restrict__ ch_std, uint32_t k0,
                                                              uint32_t k1, uint32_t epoch, uint32_t first, const float* __restrict__ eps_in,
                                                              float* __restrict__ x, long* __restrict__ y, long* __restrict__ idx_out) {
    __shared__ uint32_t s_k;
    const uint32_t j = blockIdx.x, p = first + j;                      // p < N: checked by the caller
    if (threadIdx.x == 0) {
        const uint32_t k = feistel_perm(p, N, half, epoch, k0, k1);
        s_k = k;
        if (blockIdx.y == 0) {
            y[j] = labels[k];
            if (idx_out) idx_out[j] = (long)k;
        }
    }
    __syncthreads();
    const size_t src = (size_t)s_k * per_sample, dst = (size_t)j * per_sample;
    const int groups = (per_sample + 3) >> 2;
    for (int g = blockIdx.y * DS_LANES + threadIdx.x; g < groups; g += gridDim.y * DS_LANES) {
        const int i0 = 4 * g;
        const int n = VEC || per_sample - i0 >= 4 ? 4 : per_sample - i0;
        float m[4], s[4], e[4], o[4];
        if (VEC) {
            const float4 mv = *reinterpret_cast<const float4*>(means + src + i0), sv = *reinterpret_cast<const float4*>(stds + src + i0);
            m[0] = mv.x, m[1] = mv.y, m[2] = mv.z, m[3] = mv.w;
            s[0] = sv.x, s[1] = sv.y, s[2] = sv.z, s[3] = sv.w;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) m[l] = l < n ? means[src + i0 + l] : 0.f, s[l] = l < n ? stds[src + i0 + l] : 0.f;
        }
        if (eps_in == nullptr) {
            philox_normal4((uint32_t)g, p, epoch, DS_TAG_NOISE, k0, k1, e);
        } else if (VEC) {
            const float4 ev = *reinterpret_cast<const float4*>(eps_in + dst + i0);
            e[0] = ev.x, e[1] = ev.y, e[2] = ev.z, e[3] = ev.w;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) e[l] = l < n ? eps_in[dst + i0 + l] : 0.f;
        }
        int c = i0 / hw, rem = i0 - c * hw;                            // the channel of element i0 and its offset inside it
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (l < n) {                                               // (c stays below C: element i0 + l exists)
                const float f = m[l] + e[l] * s[l];
                o[l] = (f - ch_mean[c]) / ch_std[c];
                if (++rem == hw) rem = 0, ++c;
            }
        }
        if (VEC) {
            *reinterpret_cast<float4*>(x + dst + i0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (l < n) x[dst + i0 + l] = o[l];
        }
    }
}

// half the width of the Feistel network: b = the smallest even number >= max(2, bit length of N - 1)
int feistel_half(long N) {
    int bits = 0;
    for (unsigned long v = (unsigned long)(N - 1); v; v >>= 1) ++bits;
    return bits < 2 ? 1 : (bits + 1) / 2;
}

}  // namespace

extern "C" int mapdit_philox_normal(uint64_t seed, uint32_t c1, uint32_t c2, uint32_t c3, float* out, long n, void* stream) {
    MD_CHECK(n >= 1 && n <= (1L << 34), "philox_normal: n=%ld values (1 <= n <= 2^34: the first counter word is n / 4)", n);
    MD_CHECK(out && aligned(out, 4), "philox_normal: null or unaligned pointer (out)");
    const long groups = (n + 3) / 4;
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((groups + DS_LANES - 1) / DS_LANES)), dim3(DS_LANES), 0, (hipStream_t)stream,
                       (uint32_t)seed, (uint32_t)(seed >> 32), c1, c2, c3, out, n, aligned(out, 16) ? 1 : 0);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_data_perm(uint64_t seed, uint32_t epoch, long N, long first, long count, int64_t* idx, void* stream) {
    MD_CHECK(N >= 1 && N < (1L << 32), "data_perm: N=%ld samples (1 <= N < 2^32)", N);
    MD_CHECK(count >= 1 && first >= 0 && first <= N - count, "data_perm: positions [%ld, %ld + %ld) do not lie in [0, N = %ld)", first, first, count, N);
    MD_CHECK(idx && aligned(idx, 8), "data_perm: null or unaligned pointer (idx)");
    hipLaunchKernelGGL(data_perm_kernel, dim3((unsigned)((count + DS_LANES - 1) / DS_LANES)), dim3(DS_LANES), 0, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), epoch, (uint32_t)N, feistel_half(N), first, count, (long*)idx);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_data_batch(const float* means, const float* stds, const int64_t* labels, long N, int C, int hw, const float* ch_mean,
                                 const float* ch_std, uint64_t seed, uint32_t epoch, long first, int count, const float* eps_in, float* x,
                                 int64_t* y, int64_t* idx_out, void* stream) {
    MD_CHECK(means && stds && labels && ch_mean && ch_std && x && y, "data_batch: null pointer (means, stds, labels, ch_mean, ch_std, x, y)");
    MD_CHECK(N >= 1 && N < (1L << 32), "data_batch: N=%ld samples (1 <= N < 2^32)", N);
    MD_CHECK(C >= 1 && hw >= 1, "data_batch: C=%d channels of hw=%d elements (both >= 1)", C, hw);
    MD_CHECK((long)C * hw <= 0x7fffffffL - 4, "data_batch: C * hw = %ld elements per sample exceed 2^31", (long)C * hw);
    MD_CHECK(count >= 1, "data_batch: count=%d samples (count >= 1)", count);
    MD_CHECK(first >= 0 && first <= N - count, "data_batch: positions [%ld, %ld + %d) do not lie in [0, N = %ld)", first, first, count, N);
    MD_CHECK(aligned(means, 4) && aligned(stds, 4) && aligned(ch_mean, 4) && aligned(ch_std, 4) && aligned(x, 4) && aligned(eps_in, 4) &&
                 aligned(labels, 8) && aligned(y, 8) && aligned(idx_out, 8), "data_batch: unaligned pointer");
    const int per_sample = C * hw, groups = (per_sample + 3) / 4;
    const bool vec = per_sample % 4 == 0 && aligned(means, 16) && aligned(stds, 16) && aligned(x, 16) && aligned(eps_in, 16);
    const int chunks = cdiv(groups, DS_LANES) < DS_MAX_CHUNKS ? cdiv(groups, DS_LANES) : DS_MAX_CHUNKS;
    const dim3 grid((unsigned)count, (unsigned)chunks);
    if (vec) {
        hipLaunchKernelGGL(data_batch_kernel<true>, grid, dim3(DS_LANES), 0, (hipStream_t)stream, means, stds, (const long*)labels, (uint32_t)N,
                           feistel_half(N), hw, per_sample, ch_mean, ch_std, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, (uint32_t)first, eps_in,
                           x, (long*)y, (long*)idx_out);
    } else {
        hipLaunchKernelGGL(data_batch_kernel<false>, grid, dim3(DS_LANES), 0, (hipStream_t)stream, means, stds, (const long*)labels, (uint32_t)N,
                           feistel_half(N), hw, per_sample, ch_mean, ch_std, (uint32_t)seed, (uint32_t)(seed >> 32), epoch, (uint32_t)first, eps_in,
                           x, (long*)y, (long*)idx_out);
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
