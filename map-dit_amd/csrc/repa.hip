// Representation alignment (REPA, Yu et al. 2024): the pointwise kernels of the alignment head (mapdit.h, "REPA") and the gradient-stream
// add behind mapdit_engine_set_hidden_grad.  The head's products are the library's GEMMs (repa.py sequences them); here are
//   * bias + SiLU forward and backward with the bias gradient as a two-stage column sum in a fixed order (no atomics),
//   * the negative cosine similarity of every token with its target feature, the per-sample loss and d loss / d z in one launch,
//   * out16 <- round(out16 + alpha * dh): the injected gradient, added to the operand the engine's fused residual / modulate
//     backward reads next.
// Built once per 16-bit operand format (csrc/Makefile); the fp32-only entry points exist in the bf16 build alone.
#include "common.h"

MD_NS_OPEN

// plain SiLU and its derivative with IEEE divisions: the head is a few per cent of a step and its pre-activations stay fp32
__device__ __forceinline__ float repa_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }

// pre[m][c] += bias[c] in place; act[m][c] = round16(silu(pre[m][c])) where act != nullptr.  Four elements per thread.
__global__ __launch_bounds__(256) void repa_bias_silu_fwd_kernel(float* __restrict__ pre, const float* __restrict__ bias, bf16_t* __restrict__ act,
                                                                 long n4, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)((i * 4) % C);
    const float4 b = *(const float4*)(bias + c);
    float4 v = ((float4*)pre)[i];
    v.x += b.x;
    v.y += b.y;
    v.z += b.z;
    v.w += b.w;
    ((float4*)pre)[i] = v;
    if (act) ((uint2*)act)[i] = uint2{pack16s(v.x * repa_sigmoid(v.x), v.y * repa_sigmoid(v.y)), pack16s(v.z * repa_sigmoid(v.z), v.w * repa_sigmoid(v.w))};
}

// dpre = alpha * dact * silu'(pre) (pre == nullptr: the identity's derivative, 1), stored as 16 bits where dpre16 != nullptr, and
// part[chunk][c] = the sum of the fp32 dpre over the chunk's rows.  A workgroup owns 256 columns (a lane four of them) and
// MAPDIT_REPA_PART_ROWS rows: wave w adds rows w, w + 4, ... in that order, the four wave sums are added in wave order.
__global__ __launch_bounds__(256) void repa_bias_silu_bwd_kernel(const float* __restrict__ dact, const float* __restrict__ pre, bf16_t* __restrict__ dpre16,
                                                                 float* __restrict__ part, float alpha, long M, int C) {
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + lane * 4;
    const long r0 = (long)blockIdx.y * MAPDIT_REPA_PART_ROWS;
    const long r1 = r0 + MAPDIT_REPA_PART_ROWS < M ? r0 + MAPDIT_REPA_PART_ROWS : M;
    float4 s = float4{0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        for (long r = r0 + wave; r < r1; r += 4) {
            const size_t at = (size_t)r * C + c;
            float4 d = *(const float4*)(dact + at);
            d.x *= alpha;
            d.y *= alpha;
            d.z *= alpha;
            d.w *= alpha;
            if (pre) {
                const float4 p = *(const float4*)(pre + at);
                const float s0 = repa_sigmoid(p.x), s1 = repa_sigmoid(p.y), s2 = repa_sigmoid(p.z), s3 = repa_sigmoid(p.w);
                d.x *= s0 * (1.f + p.x * (1.f - s0));
                d.y *= s1 * (1.f + p.y * (1.f - s1));
                d.z *= s2 * (1.f + p.z * (1.f - s2));
                d.w *= s3 * (1.f + p.w * (1.f - s3));
            }
            if (dpre16) *(uint2*)(dpre16 + at) = uint2{pack16(d.x, d.y), pack16(d.z, d.w)};
            s.x += d.x;
            s.y += d.y;
            s.z += d.z;
            s.w += d.w;
        }
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C) {
        float4 t = red[0][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float4 u = red[w][lane];
            t.x += u.x;
            t.y += u.y;
            t.z += u.z;
            t.w += u.w;
        }
        *(float4*)(part + (size_t)blockIdx.y * C + c) = t;
    }
}

// d rounded to fp32 with the sticky bit kept in the last place (round to odd): rounding THAT to a 16-bit format to nearest even gives
// the correctly rounded 16-bit value of d (the intermediate carries 13 / 16 bits more than the target; two would do)
__device__ __forceinline__ float repa_round_odd(double d) {
    float f = (float)d;
    if ((double)f != d && f - f == 0.f) {
        uint32_t u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) u -= 1;       // back to the truncated magnitude (f != 0 here)
        f = __uint_as_float(u | 1u);
    }
    return f;
}

// out[i] = round16(out[i] + alpha * dh[i]): the sum is formed in fp64 (the product of two fp32 values is exact there) and rounded once
__global__ __launch_bounds__(256) void repa_stream_add_kernel(bf16_t* __restrict__ out, const float* __restrict__ dh, float alpha, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const uint4 v = ((const uint4*)out)[i];
    const float4 a = ((const float4*)dh)[2 * i], b = ((const float4*)dh)[2 * i + 1];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const float d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float lo = repa_round_odd((double)up16((bf16_t)(w[e] & 0xffffu)) + (double)alpha * (double)d[2 * e]);
        const float hi = repa_round_odd((double)up16((bf16_t)(w[e] >> 16)) + (double)alpha * (double)d[2 * e + 1]);
        o[e] = (uint32_t)cvt16(lo) | ((uint32_t)cvt16(hi) << 16);
    }
    ((uint4*)out)[i] = uint4{o[0], o[1], o[2], o[3]};
}

#if MAPDIT_DT == 0
// out[c] = (accumulate ? out[c] : 0) + scale * (part[0][c] + part[1][c] + ...), the chunks in index order
__global__ __launch_bounds__(256) void repa_colsum_finish_kernel(const float* __restrict__ part, int nparts, float* __restrict__ out, float scale,
                                                                 int accumulate, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += part[(size_t)p * C + c];
    s *= scale;
    out[c] = accumulate ? out[c] + s : s;
}

__global__ __launch_bounds__(256) void repa_stream_add_f32_kernel(float* __restrict__ out, const float* __restrict__ dh, float alpha, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 v = ((float4*)out)[i];
    const float4 d = ((const float4*)dh)[i];
    v.x = fmaf(alpha, d.x, v.x);
    v.y = fmaf(alpha, d.y, v.y);
    v.z = fmaf(alpha, d.z, v.z);
    v.w = fmaf(alpha, d.w, v.w);
    ((float4*)out)[i] = v;
}

// Eight consecutive values of a feature row: fp32, or IEEE fp16 (the features file's format, whatever the engine's operand format)
template <int F16> __device__ __forceinline__ void repa_load8(const void* f, size_t at, float* v) {
    if constexpr (F16) {
        const uint4 w = *(const uint4*)((const uint16_t*)f + at);
        const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f16x2_t h = __builtin_bit_cast(f16x2_t, u[e]);
            v[2 * e] = (float)h.x;
            v[2 * e + 1] = (float)h.y;
        }
    } else {
        const float4 a = *(const float4*)((const float*)f + at), b = *(const float4*)((const float*)f + at + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}

// One workgroup per sample, a wave per token row: lane l walks columns 8 l + 512 i + (0 .. 7) in index order, the three row sums
// (|z|^2, |f|^2, <z, f>) meet in the xor butterfly.  Wave w adds the cosines of rows w, w + 4, ... in that order; the four wave sums
// are added in wave order.  Second walk over the row: dz = -(g / T) * (f^ / nz - cos * z / nz^2), nz = max(|z|, eps), f^ = f / max(|f|, eps);
// below eps the normalisation is the constant 1 / eps and only its first term is left (F.normalize's autograd).
template <int F16> __global__ __launch_bounds__(256) void repa_cos_loss_kernel(const float* __restrict__ z, const void* __restrict__ f,
                                                                               const float* __restrict__ gscale, float scale, float* __restrict__ loss,
                                                                               float* __restrict__ dz, int T, int P) {
    __shared__ float wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = blockIdx.x;
    const float eps = 1e-12f;
    const float g = (gscale ? gscale[n] * scale : scale) / (float)T;
    float acc = 0.f;
    for (int t = wave; t < T; t += 4) {
        const size_t row = ((size_t)n * T + t) * P;
        float zz = 0.f, ff = 0.f, zf = 0.f;
        for (int c = lane * 8; c < P; c += 512) {
            float fv[8];
            repa_load8<F16>(f, row + c, fv);
            const float4 a = *(const float4*)(z + row + c), b = *(const float4*)(z + row + c + 4);
            const float zv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                zz = fmaf(zv[e], zv[e], zz);
                ff = fmaf(fv[e], fv[e], ff);
                zf = fmaf(zv[e], fv[e], zf);
            }
        }
        zz = wave_sum(zz);
        ff = wave_sum(ff);
        zf = wave_sum(zf);
        const float nzr = sqrtf(zz), nfr = sqrtf(ff);
        const float nz = fmaxf(nzr, eps), nf = fmaxf(nfr, eps);
        const float cosv = (zf / nz) / nf;
        acc += cosv;
        if (dz) {
            const float kf = -g / (nz * nf);                               // coefficient of f
            const float kz = nzr >= eps ? g * cosv / (nz * nz) : 0.f;      // coefficient of z
            for (int c = lane * 8; c < P; c += 512) {
                float fv[8];
                repa_load8<F16>(f, row + c, fv);
                const float4 a = *(const float4*)(z + row + c), b = *(const float4*)(z + row + c + 4);
                *(float4*)(dz + row + c) = float4{fmaf(kz, a.x, kf * fv[0]), fmaf(kz, a.y, kf * fv[1]), fmaf(kz, a.z, kf * fv[2]), fmaf(kz, a.w, kf * fv[3])};
                *(float4*)(dz + row + c + 4) = float4{fmaf(kz, b.x, kf * fv[4]), fmaf(kz, b.y, kf * fv[5]), fmaf(kz, b.z, kf * fv[6]), fmaf(kz, b.w, kf * fv[7])};
            }
        }
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss) loss[n] = -(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / (float)T;
}
#endif

MD_NS_CLOSE

#define REPA_ALIGNED16(p) (!((uintptr_t)(p) & 15))

extern "C" int MD_SYM(repa_bias_silu_fwd)(float* pre, const float* bias, uint16_t* act, long M, int C, void* stream) {
    MD_CHECK(pre && bias, "repa_bias_silu_fwd: null argument");
    MD_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && M * C < (1L << 40), "repa_bias_silu_fwd: M=%ld, C=%d (a multiple of 8)", M, C);
    MD_CHECK(REPA_ALIGNED16(pre) && REPA_ALIGNED16(bias) && REPA_ALIGNED16(act), "repa_bias_silu_fwd: the tensors must be 16-byte aligned");
    const long n4 = M * C / 4;
    repa_bias_silu_fwd_kernel<<<cdiv(n4, 256), 256, 0, (hipStream_t)stream>>>(pre, bias, (bf16_t*)act, n4, C);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(repa_bias_silu_bwd)(const float* dact, const float* pre, uint16_t* dpre16, float* dbias, float* part, float alpha, float bias_scale,
                                          int accumulate, long M, int C, void* stream) {
    MD_CHECK(dact && dbias && part, "repa_bias_silu_bwd: null argument");
    MD_CHECK(M >= 1 && C >= 8 && C % 8 == 0 && M * C < (1L << 40), "repa_bias_silu_bwd: M=%ld, C=%d (a multiple of 8)", M, C);
    MD_CHECK(REPA_ALIGNED16(dact) && REPA_ALIGNED16(pre) && REPA_ALIGNED16(dpre16) && REPA_ALIGNED16(part),
             "repa_bias_silu_bwd: the tensors must be 16-byte aligned");
    const long nparts = (M + MAPDIT_REPA_PART_ROWS - 1) / MAPDIT_REPA_PART_ROWS;
    MD_CHECK(nparts <= 65535, "repa_bias_silu_bwd: M=%ld rows are too many for one call (%d x 65,535 at the most)", M, MAPDIT_REPA_PART_ROWS);
    const dim3 grid((unsigned)cdiv(C, 256), (unsigned)nparts);
    repa_bias_silu_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(dact, pre, (bf16_t*)dpre16, part, alpha, M, C);
    MD_LAUNCH_CHECK();
    return mapdit_repa_colsum_finish(part, (int)nparts, dbias, bias_scale, accumulate, C, stream);
}

extern "C" int MD_SYM(repa_stream_add)(uint16_t* out, const float* dh, float alpha, long n, void* stream) {
    MD_CHECK(out && dh, "repa_stream_add: null argument");
    MD_CHECK(n >= 8 && n % 8 == 0 && n < (1L << 40), "repa_stream_add: n=%ld must be a positive multiple of 8", n);
    MD_CHECK(REPA_ALIGNED16(out) && REPA_ALIGNED16(dh), "repa_stream_add: out and dh must be 16-byte aligned");
    repa_stream_add_kernel<<<cdiv(n / 8, 256), 256, 0, (hipStream_t)stream>>>((bf16_t*)out, dh, alpha, n / 8);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

#if MAPDIT_DT == 0
extern "C" int mapdit_repa_colsum_finish(const float* part, int nparts, float* out, float scale, int accumulate, int C, void* stream) {
    MD_CHECK(part && out && nparts >= 1 && C >= 1, "repa_colsum_finish: null / empty argument");
    repa_colsum_finish_kernel<<<cdiv(C, 256), 256, 0, (hipStream_t)stream>>>(part, nparts, out, scale, accumulate, C);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_repa_stream_add_f32(float* out, const float* dh, float alpha, long n, void* stream) {
    MD_CHECK(out && dh, "repa_stream_add_f32: null argument");
    MD_CHECK(n >= 4 && n % 4 == 0 && n < (1L << 40), "repa_stream_add_f32: n=%ld must be a positive multiple of 4", n);
    MD_CHECK(REPA_ALIGNED16(out) && REPA_ALIGNED16(dh), "repa_stream_add_f32: out and dh must be 16-byte aligned");
    repa_stream_add_f32_kernel<<<cdiv(n / 4, 256), 256, 0, (hipStream_t)stream>>>(out, dh, alpha, n / 4);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_repa_cos_loss(const float* z, const void* f, int f_kind, const float* gscale, float scale, float* loss, float* dz, long R, int T,
                                    int P, void* stream) {
    MD_CHECK(z && f && (loss || dz), "repa_cos_loss: null argument");
    MD_CHECK(f_kind == MAPDIT_REPA_F_F32 || f_kind == MAPDIT_REPA_F_F16, "repa_cos_loss: bad f_kind %d", f_kind);
    MD_CHECK(T >= 1 && R >= T && R % T == 0, "repa_cos_loss: R=%ld rows are no whole number of samples of T=%d tokens", R, T);
    MD_CHECK(P >= 8 && P % 8 == 0, "repa_cos_loss: P=%d must be a positive multiple of 8", P);
    MD_CHECK(R / T < (1L << 31) && R * P < (1L << 40), "repa_cos_loss: R=%ld x P=%d are too many for one call", R, P);
    MD_CHECK(REPA_ALIGNED16(z) && REPA_ALIGNED16(f) && REPA_ALIGNED16(dz), "repa_cos_loss: z, f and dz must be 16-byte aligned");
    const unsigned grid = (unsigned)(R / T);
    if (f_kind == MAPDIT_REPA_F_F16) repa_cos_loss_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(z, f, gscale, scale, loss, dz, T, P);
    else repa_cos_loss_kernel<0><<<grid, 256, 0, (hipStream_t)stream>>>(z, f, gscale, scale, loss, dz, T, P);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
#endif
