// FD-DINOv2's feature network: a plain pre-norm ViT (LayerNorm, biased linears, softmax attention, exact GELU, LayerScale) in the
// layout of the public dinov2_vit{s,b,l}14 weights (mapdit.h, "DINOv2 ViT").  Built once per 16-bit operand format (csrc/Makefile).
// Activations between the kernels are 16-bit, accumulation is fp32 and THE RESIDUAL STREAM IS FP32: DINOv2's residual carries
// outliers of a few hundred, which a 16-bit stream would round to steps of 0.25 and more.
//
// Linears: conv.hip's implicit GEMM (common.h, md_conv_t) as a 1 x 1 convolution over M "images" of one pixel each: bias, an fp32
// or 16-bit store, row and column guards.  The 128-wide tile where Cout % 128 == 0, the 64-wide one else; the two give the same bits,
// and the K order of an output element does not depend on M, so a sample alone and in a batch gives the same bits.
//
// Attention (head_dim 64, any T >= 2): a workgroup of four waves owns 64 query rows of one (sample, head), a wave 16 of them.  Keys
// are streamed in tiles of 64 through LDS with an online softmax.  Both products are v_mfma_f32_16x16x32 in the SWAPPED orientation:
// S^T = K Q^T puts a query on the lane (column) and the tile's keys in the registers, so the row maximum and sum are in-register
// plus two lane exchanges, and P^T feeds O^T = V^T P^T as the B operand with no lane movement.  V is staged transposed, its keys in
// the order the P fragment holds them.  Query rows and key columns past T are zeros that are never loaded; masked scores are -inf.
#include "common.h"

MD_NS_OPEN

// ---- prepare: antialiased bicubic resize + ImageNet normalisation + patch rows -------------------------------------------------------
// Keys cubic, a = -0.5
__device__ __forceinline__ float vit_cubic(float x) {
    x = fabsf(x);
    if (x < 1.f) return (1.5f * x - 2.5f) * x * x + 1.f;
    if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * -0.5f;
    return 0.f;
}

// One axis of F.interpolate(mode="bicubic", antialias=True, align_corners=False) for destination index d of S from a source of I:
// scale = I / S, centre = scale (d + 1/2), support = 2 max(scale, 1), taps [lo, hi) = [max(0, trunc(centre - support + 1/2)),
// min(I, trunc(centre + support + 1/2))), weight of tap t = cubic((t + 1/2 - centre) / max(scale, 1)), normalised by the taps' sum.
// Everything is a ratio of integers over 2 S (or 2 I): the tap range is exact and a weight's argument is one fp32 division.
struct VitAxis {
    int lo, hi;
    long c2;        // (2 d + 1) I = 2 S centre
    int S;
    float den;      // 2 max(I, S)
    __device__ __forceinline__ float w(int t) const { return vit_cubic((float)((long)(2 * t + 1) * S - c2) / den); }
};
__device__ __forceinline__ VitAxis vit_axis(int d, int I, int S) {
    VitAxis a;
    a.S = S;
    a.c2 = (long)(2 * d + 1) * I;
    const long sup = 4L * (I > S ? I : S);                  // 2 S support
    const long ln = a.c2 - sup + S, hn = a.c2 + sup + S;      // 2 S (centre -+ support + 1/2)
    a.lo = ln <= 0 ? 0 : (int)(ln / (2L * S));
    const long h = hn / (2L * S);
    a.hi = h < I ? (int)h : I;
    a.den = (float)(2L * (I > S ? I : S));
    return a;
}

// out 16-bit [N * P, Kp], P = (S / 14)^2, row = (n, gy, gx), column k = c * 196 + py * 14 + px (the flattening of a [D, 3, 14, 14]
// convolution weight), columns [588, Kp) zero.  The horizontal pass of a source row is summed first, then the rows (torch's order),
// on pixel values in 0 .. 255; then / 255, - mean, / std.  u8 == 0: img fp32 [N, 3, H, W] in [-1, 1], taken to 0 .. 255 as (v + 1) * 127.5.
__global__ __launch_bounds__(256) void vit_prepare_kernel(const void* __restrict__ img, int u8, bf16_t* __restrict__ out, long total, int H, int W,
                                                          int S, int Kp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % Kp);
    if (k >= 588) {
        out[idx] = 0;
        return;
    }
    const long row = idx / Kp;
    const int g = S / 14, P = g * g;
    const int p = (int)(row % P);
    const long n = row / P;
    const int c = k / 196, py = (k % 196) / 14, px = k % 14;
    const int y = (p / g) * 14 + py, x = (p % g) * 14 + px;
    const VitAxis ay = vit_axis(y, H, S), ax = vit_axis(x, W, S);
    float ty = 0.f, tx = 0.f;
    for (int t = ay.lo; t < ay.hi; ++t) ty += ay.w(t);
    for (int t = ax.lo; t < ax.hi; ++t) tx += ax.w(t);
    float acc = 0.f;
    for (int yy = ay.lo; yy < ay.hi; ++yy) {
        float r = 0.f;
        if (u8) {
            const uint8_t* b = (const uint8_t*)img + (((size_t)n * H + yy) * W) * 3 + c;
            for (int xx = ax.lo; xx < ax.hi; ++xx) r = fmaf(ax.w(xx) / tx, (float)b[(size_t)xx * 3], r);
        } else {
            const float* b = (const float*)img + (((size_t)n * 3 + c) * H + yy) * W;
            for (int xx = ax.lo; xx < ax.hi; ++xx) r = fmaf(ax.w(xx) / tx, (b[xx] + 1.f) * 127.5f, r);
        }
        acc = fmaf(ay.w(yy) / ty, r, acc);
    }
    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, sd = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
    out[idx] = cvt16s((acc / 255.f - mean) / sd);
}

// ---- LayerNorm: fp32 rows -> 16-bit (or fp32) ------------------------------------------------------------------------------------------
// One wave per row, two passes in fp32: lane l sums elements 4 l + 256 i + (0 .. 3) in index order, the 64 partial sums meet in the
// xor butterfly (a fixed tree); the mean, then the same walk over (x - mean)^2.  Nothing depends on the number of rows.
__global__ __launch_bounds__(256) void vit_layernorm_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w, const float* __restrict__ b,
                                                            float eps, void* __restrict__ out, int out16, long M, int D) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (size_t)row * ldx;
    float s = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4*)(xr + d);
        s += v.x;
        s += v.y;
        s += v.z;
        s += v.w;
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4*)(xr + d);
        const float a0 = v.x - mean, a1 = v.y - mean, a2 = v.z - mean, a3 = v.w - mean;
        q = fmaf(a0, a0, q);
        q = fmaf(a1, a1, q);
        q = fmaf(a2, a2, q);
        q = fmaf(a3, a3, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4*)(xr + d), g = *(const float4*)(w + d), h = *(const float4*)(b + d);
        const float o0 = fmaf((v.x - mean) * rstd, g.x, h.x), o1 = fmaf((v.y - mean) * rstd, g.y, h.y);
        const float o2 = fmaf((v.z - mean) * rstd, g.z, h.z), o3 = fmaf((v.w - mean) * rstd, g.w, h.w);
        if (out16) *(uint2*)((bf16_t*)out + (size_t)row * D + d) = uint2{pack16s(o0, o1), pack16s(o2, o3)};
        else *(float4*)((float*)out + (size_t)row * D + d) = float4{o0, o1, o2, o3};
    }
}

// ---- attention -----------------------------------------------------------------------------------------------------------------------
constexpr int VA_LD = 72;        // LDS row of 64 elements + 8: 144 B, 16-byte aligned, consecutive rows 4 banks apart

__global__ __launch_bounds__(256) void vit_attn_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T, int Hn) {
    __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * VA_LD];       // [key][dim]
    __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * VA_LD];       // [dim][key slot]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int h = blockIdx.y, n = blockIdx.z;
    const int D = Hn * 64;
    const size_t ld = (size_t)3 * D;
    const bf16_t* base = qkv + (size_t)n * T * ld + (size_t)h * 64;      // q of the head; k at + D, v at + 2 D
    const int qrow = blockIdx.x * 64 + wave * 16 + r;

    // Q as the B operand: column = query r, k = dims 32 ks + 8 q + (0 .. 7); a row past T is zeros, never an address
    bf16x8_t qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (qrow < T) v = *(const uint4*)(base + (size_t)qrow * ld + ks * 32 + q * 8);
        qf[ks] = __builtin_bit_cast(bf16x8_t, v);
    }

    f32x4_t o[4];                // o[dt][e]: dim 16 dt + 4 q + e of query r
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    // staging role: key srow of the tile, dims [sc, sc + 16).  Key 16 j + 4 qq + e goes to slot 32 (j >> 1) + 8 qq + 4 (j & 1) + e:
    // the eight keys lane group qq holds of score tiles 2 kk and 2 kk + 1 are the eight consecutive slots of PV's k-step kk
    const int srow = tid >> 2, sc = (tid & 3) * 16;
    const int sj = srow >> 4, spos = (sj >> 1) * 32 + ((srow & 15) >> 2) * 8 + (sj & 1) * 4 + (srow & 3);

    for (int k0 = 0; k0 < T; k0 += 64) {
        const int key = k0 + srow;
        uint4 kv[2], vv[2];
        kv[0] = kv[1] = vv[0] = vv[1] = uint4{0u, 0u, 0u, 0u};
        if (key < T) {
            const uint4* kp = (const uint4*)(base + (size_t)key * ld + D + sc);
            const uint4* vp = (const uint4*)(base + (size_t)key * ld + 2 * (size_t)D + sc);
            kv[0] = kp[0];
            kv[1] = kp[1];
            vv[0] = vp[0];
            vv[1] = vp[1];
        }
        __syncthreads();         // every wave has left the previous tile
        *(uint4*)(&Ks[srow * VA_LD + sc]) = kv[0];
        *(uint4*)(&Ks[srow * VA_LD + sc + 8]) = kv[1];
        const uint32_t vw[8] = {vv[0].x, vv[0].y, vv[0].z, vv[0].w, vv[1].x, vv[1].y, vv[1].z, vv[1].w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            Vt[(sc + 2 * i) * VA_LD + spos] = (bf16_t)(vw[i] & 0xffffu);
            Vt[(sc + 2 * i + 1) * VA_LD + spos] = (bf16_t)(vw[i] >> 16);
        }
        __syncthreads();

        // S^T = K Q^T: s[j][e] = score of key k0 + 16 j + 4 q + e with query r
        f32x4_t s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8_t a = *(const bf16x8_t*)(&Ks[(j * 16 + r) * VA_LD + ks * 32 + q * 8]);
                s[j] = MFMA16(a, qf[ks], s[j]);
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = k0 + j * 16 + q * 4 + e < T ? s[j][e] * 0.125f : -INFINITY;
                s[j][e] = v;
                tmax = fmaxf(tmax, v);
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);                     // finite: key k0 is inside T
        const float alpha = __expf(m - mn);                  // (0 on the first tile)
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pv = __expf(s[j][e] - mn);       // a masked key: exp(-inf) = 0
                s[j][e] = pv;
                ps += pv;
            }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l = fmaf(l, alpha, ps);
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[dt][e] = o[dt][e] * alpha;
        // O^T += V^T P^T
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const uint4 pw = uint4{pack16(s[2 * kk][0], s[2 * kk][1]), pack16(s[2 * kk][2], s[2 * kk][3]), pack16(s[2 * kk + 1][0], s[2 * kk + 1][1]),
                                   pack16(s[2 * kk + 1][2], s[2 * kk + 1][3])};
            const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8_t a = *(const bf16x8_t*)(&Vt[(dt * 16 + r) * VA_LD + kk * 32 + q * 8]);
                o[dt] = MFMA16(a, pf, o[dt]);
            }
        }
    }

    if (qrow < T) {
        const float inv = 1.f / l;
        bf16_t* orow = out + ((size_t)n * T + qrow) * D + (size_t)h * 64 + q * 4;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *(uint2*)(orow + dt * 16) = uint2{pack16s(o[dt][0] * inv, o[dt][1] * inv), pack16s(o[dt][2] * inv, o[dt][3] * inv)};
    }
}

// ---- pointwise -------------------------------------------------------------------------------------------------------------------------
// exact GELU 0.5 x (1 + erf(x / sqrt 2)) in fp32, written 0.5 x erfc(-x / sqrt 2): the same function without the cancellation of 1 + erf
// for negative x.  Eight 16-bit elements per thread; in may be out
__global__ __launch_bounds__(256) void vit_gelu_kernel(const bf16_t* in, bf16_t* out, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const uint4 v = ((const uint4*)in)[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float a = lo16(w[e]), b = hi16(w[e]);
        const float ga = 0.5f * a * erfcf(a * -0.70710678118654752440f), gb = 0.5f * b * erfcf(b * -0.70710678118654752440f);
        o[e] = pack16s(ga, gb);
    }
    ((uint4*)out)[i] = uint4{o[0], o[1], o[2], o[3]};
}

// x[m][d] += gamma[d] * y[m][d]: one fma per element, four per thread
template <int Y16> __global__ __launch_bounds__(256) void vit_residual_kernel(float* __restrict__ x, const void* __restrict__ y, const float* __restrict__ gamma,
                                                                              long n4, int D) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int d = (int)((i * 4) % D);
    const float4 g = *(const float4*)(gamma + d);
    float4 xv = ((float4*)x)[i];
    float y0, y1, y2, y3;
    if constexpr (Y16) {
        const uint2 w = ((const uint2*)y)[i];
        y0 = lo16(w.x);
        y1 = hi16(w.x);
        y2 = lo16(w.y);
        y3 = hi16(w.y);
    } else {
        const float4 w = ((const float4*)y)[i];
        y0 = w.x;
        y1 = w.y;
        y2 = w.z;
        y3 = w.w;
    }
    xv.x = fmaf(g.x, y0, xv.x);
    xv.y = fmaf(g.y, y1, xv.y);
    xv.z = fmaf(g.z, y2, xv.z);
    xv.w = fmaf(g.w, y3, xv.w);
    ((float4*)x)[i] = xv;
}

#if MAPDIT_DT == 0
// tokens fp32 [N, T, D]: row 0 = cls + pos[0], row 1 + p = patch[n * P + p] + pos[1 + p]; four elements per thread
__global__ __launch_bounds__(256) void vit_embed_kernel(const float* __restrict__ patch, const float* __restrict__ cls, const float* __restrict__ pos,
                                                        float* __restrict__ out, long n4, int T, int D) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const long e = i * 4;
    const int d = (int)(e % D);
    const long row = e / D;
    const int t = (int)(row % T);
    const long n = row / T;
    const float4 a = t == 0 ? *(const float4*)(cls + d) : *(const float4*)(patch + ((size_t)n * (T - 1) + (t - 1)) * D + d);
    const float4 b = *(const float4*)(pos + (size_t)t * D + d);
    ((float4*)out)[i] = float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
#endif

MD_NS_CLOSE

// ---- entry points ------------------------------------------------------------------------------------------------------------------
#define VIT_ALIGNED16(p) (!((uintptr_t)(p) & 15))

extern "C" int MD_SYM(vit_prepare)(const void* images, int img_kind, uint16_t* rows, int N, int H, int W, int size, void* stream) {
    MD_CHECK(images && rows, "vit_prepare: null argument");
    MD_CHECK(img_kind == MAPDIT_VIT_IMG_U8_NHWC || img_kind == MAPDIT_VIT_IMG_F32_NCHW, "vit_prepare: bad img_kind %d", img_kind);
    MD_CHECK(N >= 1, "vit_prepare: N=%d must be at least 1", N);
    MD_CHECK(H >= 8 && W >= 8, "vit_prepare: images of %d x %d (8 x 8 at the least)", H, W);
    MD_CHECK(H < (1 << 20) && W < (1 << 20), "vit_prepare: images of %d x %d are too large (below 2^20 each way)", H, W);
    MD_CHECK(size >= MAPDIT_VIT_PATCH && size % MAPDIT_VIT_PATCH == 0 && size <= 14 * 1024, "vit_prepare: size=%d is no multiple of the patch (%d) up to %d",
             size, MAPDIT_VIT_PATCH, 14 * 1024);
    const long P = (long)(size / MAPDIT_VIT_PATCH) * (size / MAPDIT_VIT_PATCH), total = (long)N * P * MAPDIT_VIT_PATCH_K;
    MD_CHECK(total < (1L << 38) && (long)N * H * W * 3 < (1L << 40), "vit_prepare: %ld elements are too many for one call", total);
    vit_prepare_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(images, img_kind == MAPDIT_VIT_IMG_U8_NHWC, (bf16_t*)rows, total, H, W, size,
                                                                         MAPDIT_VIT_PATCH_K);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vit_linear)(const uint16_t* in, const uint16_t* w, const float* bias, void* out, int out_kind, long M, int Cin, int Cout,
                                  void* stream) {
    MD_CHECK(in && w && bias && out, "vit_linear: null argument");
    MD_CHECK(M >= 1 && M < (1L << 31) && Cin >= 16 && Cout >= 16, "vit_linear: M=%ld, Cin=%d, Cout=%d (M in 1 .. 2^31 - 1, 16 channels at the least)", M, Cin,
             Cout);
    MD_CHECK(Cin % 16 == 0 && Cout % 16 == 0, "vit_linear: Cin=%d and Cout=%d must be multiples of 16", Cin, Cout);
    MD_CHECK(out_kind == MAPDIT_VIT_OUT_F32 || out_kind == MAPDIT_VIT_OUT_16, "vit_linear: bad out_kind %d", out_kind);
    MD_CHECK(VIT_ALIGNED16(in) && VIT_ALIGNED16(w) && VIT_ALIGNED16(out), "vit_linear: in, w and out must be 16-byte aligned");
    // M images of 1 x 1: the staged row's sample is m itself
    const md_conv_t p{in, (const bf16_t*)w, bias, nullptr, out, MAPDIT_VAE_IN_16, out_kind == MAPDIT_VIT_OUT_16 ? MAPDIT_VAE_OUT_16 : MAPDIT_VAE_OUT_F32,
                      1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1, Cin, Cout, Cin, M, Cout, 0, 0};
    return MD_SYM(conv_launch)("vit_linear", &p, Cout % 128 == 0 ? MD_CONV_128 : MD_CONV_64, stream);
}

#if MAPDIT_DT == 0
extern "C" int mapdit_vit_embed(const float* patch, const float* cls, const float* pos, float* tokens, int N, int T, int D, void* stream) {
    MD_CHECK(patch && cls && pos && tokens, "vit_embed: null argument");
    MD_CHECK(N >= 1 && T >= 2 && D >= 4 && D % 4 == 0, "vit_embed: N=%d, T=%d (2 at the least), D=%d (a multiple of 4)", N, T, D);
    MD_CHECK(VIT_ALIGNED16(patch) && VIT_ALIGNED16(cls) && VIT_ALIGNED16(pos) && VIT_ALIGNED16(tokens), "vit_embed: the tensors must be 16-byte aligned");
    const long n4 = (long)N * T * D / 4;
    MD_CHECK(n4 < (1L << 36), "vit_embed: %ld elements are too many for one call", n4 * 4);
    vit_embed_kernel<<<cdiv(n4, 256), 256, 0, (hipStream_t)stream>>>(patch, cls, pos, tokens, n4, T, D);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
#endif

extern "C" int MD_SYM(vit_layernorm)(const float* x, long ldx, const float* w, const float* b, float eps, void* out, int out_kind, long M, int D,
                                     void* stream) {
    MD_CHECK(x && w && b && out, "vit_layernorm: null argument");
    MD_CHECK(M >= 1 && M < (1L << 31) && D >= 4 && D % 4 == 0 && D <= 65536, "vit_layernorm: M=%ld, D=%d (a multiple of 4 up to 65,536)", M, D);
    MD_CHECK(ldx >= D && ldx % 4 == 0, "vit_layernorm: ldx=%ld must be a multiple of 4 and at least D=%d", ldx, D);
    MD_CHECK(eps >= 0.f, "vit_layernorm: eps must not be negative");
    MD_CHECK(out_kind == MAPDIT_VIT_OUT_F32 || out_kind == MAPDIT_VIT_OUT_16, "vit_layernorm: bad out_kind %d", out_kind);
    MD_CHECK(VIT_ALIGNED16(x) && VIT_ALIGNED16(w) && VIT_ALIGNED16(b) && VIT_ALIGNED16(out), "vit_layernorm: the tensors must be 16-byte aligned");
    vit_layernorm_kernel<<<cdiv(M, 4), 256, 0, (hipStream_t)stream>>>(x, ldx, w, b, eps, out, out_kind == MAPDIT_VIT_OUT_16, M, D);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vit_attention)(const uint16_t* qkv, uint16_t* out, int N, int T, int heads, int head_dim, void* stream) {
    MD_CHECK(qkv && out, "vit_attention: null argument");
    MD_CHECK(head_dim == 64, "vit_attention: head_dim=%d; the softmax attention kernel is built for head_dim 64 only", head_dim);
    MD_CHECK(T >= 2, "vit_attention: T=%d tokens; a ViT sequence has its CLS token and one patch at the least (T >= 2)", T);
    MD_CHECK(N >= 1 && N <= 65535 && heads >= 1 && heads <= 65535, "vit_attention: N=%d and heads=%d must lie in 1 .. 65,535", N, heads);
    MD_CHECK((long)N * T < (1L << 31) && T <= (1 << 22), "vit_attention: N=%d x T=%d rows are too many for one call", N, T);
    MD_CHECK(VIT_ALIGNED16(qkv) && VIT_ALIGNED16(out), "vit_attention: qkv and out must be 16-byte aligned");
    const dim3 grid((unsigned)cdiv(T, 64), (unsigned)heads, (unsigned)N);
    vit_attn_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)qkv, (bf16_t*)out, T, heads);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vit_gelu)(const uint16_t* in, uint16_t* out, long n, void* stream) {
    MD_CHECK(in && out, "vit_gelu: null argument");
    MD_CHECK(n >= 8 && n % 8 == 0 && n < (1L << 40), "vit_gelu: n=%ld must be a positive multiple of 8", n);
    MD_CHECK(VIT_ALIGNED16(in) && VIT_ALIGNED16(out), "vit_gelu: in and out must be 16-byte aligned");
    vit_gelu_kernel<<<cdiv(n / 8, 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)in, (bf16_t*)out, n / 8);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vit_residual)(float* x, const void* y, int y_kind, const float* gamma, long M, int D, void* stream) {
    MD_CHECK(x && y && gamma, "vit_residual: null argument");
    MD_CHECK(M >= 1 && D >= 4 && D % 4 == 0 && M * D < (1L << 40), "vit_residual: M=%ld, D=%d (a multiple of 4)", M, D);
    MD_CHECK(y_kind == MAPDIT_VIT_OUT_F32 || y_kind == MAPDIT_VIT_OUT_16, "vit_residual: bad y_kind %d", y_kind);
    MD_CHECK(VIT_ALIGNED16(x) && VIT_ALIGNED16(y) && VIT_ALIGNED16(gamma), "vit_residual: the tensors must be 16-byte aligned");
    const long n4 = M * D / 4;
    if (y_kind == MAPDIT_VIT_OUT_16) vit_residual_kernel<1><<<cdiv(n4, 256), 256, 0, (hipStream_t)stream>>>(x, y, gamma, n4, D);
    else vit_residual_kernel<0><<<cdiv(n4, 256), 256, 0, (hipStream_t)stream>>>(x, y, gamma, n4, D);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

// ---- the network -------------------------------------------------------------------------------------------------------------------
namespace {
struct VitPlan {
    int g, P, T;
    long M;
    size_t off_rows, off_x, off_y, off_h, off_a, off_qkv, off_f, total;
};

int vit_plan(const mapdit_vit_config_t* c, int N, VitPlan* pl) {
    MD_CHECK(c, "vit: null config");
    MD_CHECK(N >= 1, "vit: N=%d must be at least 1", N);
    MD_CHECK(c->patch == MAPDIT_VIT_PATCH, "vit: patch=%d; the patch rows are packed for patch %d only", c->patch, MAPDIT_VIT_PATCH);
    MD_CHECK(c->image_size >= c->patch && c->image_size % c->patch == 0 && c->image_size <= 14 * 128,
             "vit: image_size=%d is no multiple of the patch (%d) in %d .. %d", c->image_size, c->patch, c->patch, 14 * 128);
    MD_CHECK(c->heads >= 1 && c->dim == 64 * c->heads, "vit: dim=%d with %d heads is no head_dim 64 (dim must equal 64 * heads)", c->dim, c->heads);
    MD_CHECK(c->dim % 16 == 0 && c->mlp_dim >= 16 && c->mlp_dim % 16 == 0, "vit: dim=%d and mlp_dim=%d must be multiples of 16", c->dim, c->mlp_dim);
    MD_CHECK(c->depth >= 1 && c->depth <= MAPDIT_VIT_MAX_DEPTH, "vit: depth=%d (1 .. %d)", c->depth, MAPDIT_VIT_MAX_DEPTH);
    MD_CHECK(c->ln_eps >= 0.f, "vit: ln_eps must not be negative");
    pl->g = c->image_size / c->patch;
    pl->P = pl->g * pl->g;
    pl->T = pl->P + 1;
    pl->M = (long)N * pl->T;
    const long widest = c->mlp_dim > 3 * c->dim ? c->mlp_dim : 3 * c->dim;
    MD_CHECK(N <= 65535 && pl->M * widest < (1L << 36), "vit: N=%d images of %d tokens are too many for one call", N, pl->T);
    const size_t M = (size_t)pl->M, D = (size_t)c->dim;
    size_t o = 0;
    pl->off_rows = o; o += md_up256((size_t)N * pl->P * MAPDIT_VIT_PATCH_K * 2);
    pl->off_x = o; o += md_up256(M * D * 4);
    pl->off_y = o; o += md_up256(M * D * 4);            // a branch's fp32 output; first the patch-embed linear's
    pl->off_h = o; o += md_up256(M * D * 2);
    pl->off_a = o; o += md_up256(M * D * 2);
    pl->off_qkv = o; o += md_up256(M * 3 * D * 2);
    pl->off_f = o; o += md_up256(M * (size_t)c->mlp_dim * 2);
    pl->total = o;
    return MAPDIT_OK;
}
}  // namespace

#if MAPDIT_DT == 0
extern "C" size_t mapdit_vit_workspace_bytes(const mapdit_vit_config_t* cfg, int N) {
    VitPlan pl;
    return vit_plan(cfg, N, &pl) == MAPDIT_OK ? pl.total : 0;
}
#endif

// The walk both outputs share: everything up to the residual stream x fp32 [N * T, dim] in front of the final LayerNorm (*xout).
static int MD_TU(vit_walk)(const char* who, const mapdit_vit_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H, int W,
                           const void* out, void* workspace, size_t ws_bytes, void* stream, VitPlan* plan, float** xout) {
    VitPlan& pl = *plan;
    MD_TRY(vit_plan(cfg, N, &pl));
    MD_CHECK(wt && images && out && workspace, "%s: null argument", who);
    MD_CHECK(img_kind == MAPDIT_VIT_IMG_U8_NHWC || img_kind == MAPDIT_VIT_IMG_F32_NCHW, "%s: bad img_kind %d", who, img_kind);
    MD_CHECK(H >= 8 && W >= 8, "%s: images of %d x %d (8 x 8 at the least)", who, H, W);
    MD_CHECK(ws_bytes >= pl.total, "%s: workspace of %zu bytes, %zu needed (mapdit_vit_workspace_bytes)", who, ws_bytes, pl.total);
    MD_CHECK(!((uintptr_t)workspace & 255), "%s: the workspace must be 256-byte aligned", who);
    MD_CHECK(VIT_ALIGNED16(out), "%s: the output must be 16-byte aligned", who);
    const int nw = MAPDIT_VIT_W_GLOBAL + cfg->depth * MAPDIT_VIT_W_BLOCK;
    for (int i = 0; i < nw; ++i) MD_CHECK(wt[i] && VIT_ALIGNED16(wt[i]), "%s: weight slot %d is null or not 16-byte aligned", who, i);
    char* ws = (char*)workspace;
    uint16_t* rows = (uint16_t*)(ws + pl.off_rows);
    float* x = (float*)(ws + pl.off_x);
    float* y = (float*)(ws + pl.off_y);
    uint16_t* hb = (uint16_t*)(ws + pl.off_h);
    uint16_t* ab = (uint16_t*)(ws + pl.off_a);
    uint16_t* qkv = (uint16_t*)(ws + pl.off_qkv);
    uint16_t* fb = (uint16_t*)(ws + pl.off_f);
    const int D = cfg->dim, F = cfg->mlp_dim, T = pl.T;
    const long M = pl.M;
    const int k16 = MAPDIT_VIT_OUT_16, k32 = MAPDIT_VIT_OUT_F32;

    MD_TRY(MD_SYM(vit_prepare)(images, img_kind, rows, N, H, W, cfg->image_size, stream));
    MD_TRY(MD_SYM(vit_linear)(rows, (const uint16_t*)wt[MAPDIT_VIT_W_PATCH], (const float*)wt[MAPDIT_VIT_W_PATCH_BIAS], y, k32, (long)N * pl.P,
                              MAPDIT_VIT_PATCH_K, D, stream));
    MD_TRY(mapdit_vit_embed(y, (const float*)wt[MAPDIT_VIT_W_CLS], (const float*)wt[MAPDIT_VIT_W_POS], x, N, T, D, stream));
    for (int b = 0; b < cfg->depth; ++b) {
        const void* const* w = wt + MAPDIT_VIT_W_GLOBAL + b * MAPDIT_VIT_W_BLOCK;
        MD_TRY(MD_SYM(vit_layernorm)(x, D, (const float*)w[MAPDIT_VIT_B_LN1], (const float*)w[MAPDIT_VIT_B_LN1_BIAS], cfg->ln_eps, hb, k16, M, D, stream));
        MD_TRY(MD_SYM(vit_linear)(hb, (const uint16_t*)w[MAPDIT_VIT_B_QKV], (const float*)w[MAPDIT_VIT_B_QKV_BIAS], qkv, k16, M, D, 3 * D, stream));
        MD_TRY(MD_SYM(vit_attention)(qkv, ab, N, T, cfg->heads, 64, stream));
        MD_TRY(MD_SYM(vit_linear)(ab, (const uint16_t*)w[MAPDIT_VIT_B_PROJ], (const float*)w[MAPDIT_VIT_B_PROJ_BIAS], y, k32, M, D, D, stream));
        MD_TRY(MD_SYM(vit_residual)(x, y, k32, (const float*)w[MAPDIT_VIT_B_LS1], M, D, stream));
        MD_TRY(MD_SYM(vit_layernorm)(x, D, (const float*)w[MAPDIT_VIT_B_LN2], (const float*)w[MAPDIT_VIT_B_LN2_BIAS], cfg->ln_eps, hb, k16, M, D, stream));
        MD_TRY(MD_SYM(vit_linear)(hb, (const uint16_t*)w[MAPDIT_VIT_B_FC1], (const float*)w[MAPDIT_VIT_B_FC1_BIAS], fb, k16, M, D, F, stream));
        MD_TRY(MD_SYM(vit_gelu)(fb, fb, M * F, stream));
        MD_TRY(MD_SYM(vit_linear)(fb, (const uint16_t*)w[MAPDIT_VIT_B_FC2], (const float*)w[MAPDIT_VIT_B_FC2_BIAS], y, k32, M, F, D, stream));
        MD_TRY(MD_SYM(vit_residual)(x, y, k32, (const float*)w[MAPDIT_VIT_B_LS2], M, D, stream));
    }
    *xout = x;
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vit_features)(const mapdit_vit_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H, int W,
                                    float* feat, void* workspace, size_t ws_bytes, void* stream) {
    VitPlan pl;
    float* x = nullptr;
    MD_TRY(MD_TU(vit_walk)("vit_features", cfg, wt, images, img_kind, N, H, W, feat, workspace, ws_bytes, stream, &pl, &x));
    // the final LayerNorm on the CLS rows alone (LayerNorm is per row): row n * T of x -> feat[n]
    return MD_SYM(vit_layernorm)(x, (long)pl.T * cfg->dim, (const float*)wt[MAPDIT_VIT_W_NORM], (const float*)wt[MAPDIT_VIT_W_NORM_BIAS], cfg->ln_eps, feat,
                                 MAPDIT_VIT_OUT_F32, N, cfg->dim, stream);
}

// The same walk with the final LayerNorm on EVERY row: tokens [N, T, dim], row 0 of a sample its CLS token (the bits of vit_features
// with an fp32 output: the LayerNorm is one wave per row and knows nothing of the other rows), rows 1 + p the patches in grid order.
extern "C" int MD_SYM(vit_tokens)(const mapdit_vit_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H, int W,
                                  void* tokens, int out_kind, void* workspace, size_t ws_bytes, void* stream) {
    MD_CHECK(out_kind == MAPDIT_VIT_OUT_F32 || out_kind == MAPDIT_VIT_OUT_16, "vit_tokens: bad out_kind %d", out_kind);
    VitPlan pl;
    float* x = nullptr;
    MD_TRY(MD_TU(vit_walk)("vit_tokens", cfg, wt, images, img_kind, N, H, W, tokens, workspace, ws_bytes, stream, &pl, &x));
    return MD_SYM(vit_layernorm)(x, cfg->dim, (const float*)wt[MAPDIT_VIT_W_NORM], (const float*)wt[MAPDIT_VIT_W_NORM_BIAS], cfg->ln_eps, tokens, out_kind,
                                 pl.M, cfg->dim, stream);
}
