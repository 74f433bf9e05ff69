// FID's feature network (the 2015 Inception-v3 in the layout of the pt_inception-2015-12-05 port, BatchNorm folded into the
// convolutions) and the fp64 feature statistics (mapdit.h, "Inception / FID").  Built once per 16-bit operand format (csrc/Makefile).
// Activations are 16-bit NHWC between the layers (a convolution rounds its input to the operand format anyway; max pooling commutes
// with that rounding, the average pool rounds once more); the image at 299 x 299 and the last block's output are fp32.
// mapdit_inc_features_tap is the same walk with one copy kernel after Mixed_6d: sFID's spatial features, the first 7 channels of
// that block's branch1x1 unit, widened to fp32 into the caller's buffer (no workspace of its own).
//
// Convolution: conv.hip's kernels (common.h, md_conv_t) with kh x kw taps, stride, pad_h / pad_w, ReLU and a store into a channel
// slice.  Cin is a multiple of 16 and of nothing larger (48, 80, 288 ...) and Cout a multiple of 16, not of 64: the 16-channel K
// granules and the row / column guards of the 64-wide tile are what these layers need.
#include "common.h"

MD_NS_OPEN

// ---- pooling ----------------------------------------------------------------------------------------------------------------------
// The three 3 x 3 forms, one thread per output element, taps in (ky, kx) order over the in-image taps only: the stride-2 maximum
// without padding (every tap is inside), the stride-1 pad-1 average that divides by the COUNT OF IN-IMAGE TAPS (count_include_pad =
// False: 4 at a corner, 6 on an edge, 9 inside; IEEE division), and the stride-1 pad-1 maximum (padding never wins).  A NaN propagates.
__device__ __forceinline__ float inc_load(const void* in, int in_f32, size_t e) { return in_f32 ? ((const float*)in)[e] : up16(((const bf16_t*)in)[e]); }

__global__ __launch_bounds__(256) void inc_pool_kernel(const void* __restrict__ in, int in_f32, void* __restrict__ out, int out16, long total,
                                                       int H, int W, int C, int Ho, int Wo, int mode, int ld, int coff) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long m = idx / C;
    const int hw = Ho * Wo;
    const int n = (int)(m / hw), rem = (int)(m % hw), y = rem / Wo, x = rem % Wo;
    const int st = mode == MAPDIT_INC_POOL_MAX_S2 ? 2 : 1, pad = mode == MAPDIT_INC_POOL_MAX_S2 ? 0 : 1;
    const bool avg = mode == MAPDIT_INC_POOL_AVG;
    float a = avg ? 0.f : -INFINITY;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y * st + ky - pad;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = x * st + kx - pad;
            if (xx < 0 || xx >= W) continue;
            const float v = inc_load(in, in_f32, (((size_t)n * H + yy) * W + xx) * C + c);
            if (avg) a += v;
            else a = (v > a || v != v) ? v : a;
            ++cnt;
        }
    }
    if (avg) a = a / (float)cnt;
    const size_t o = (size_t)m * ld + coff + c;
    if (out16) ((bf16_t*)out)[o] = cvt16s(a);
    else ((float*)out)[o] = a;
}

// [N, HW, C] -> fp32 [N, C]: one thread per (n, c), a serial fp32 sum in pixel order, IEEE division by HW
__global__ __launch_bounds__(256) void inc_global_avg_kernel(const void* __restrict__ in, int in_f32, float* __restrict__ out, long total, int HW, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long n = idx / C;
    float a = 0.f;
    for (int i = 0; i < HW; ++i) a += inc_load(in, in_f32, ((size_t)n * HW + i) * C + c);
    out[idx] = a / (float)HW;
}

// The spatial tap: channels [0, ct) of a 16-bit [pixels, C] activation -> fp32 [pixels, ct], one thread per output element
__global__ __launch_bounds__(256) void inc_tap_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, long total, int C, int ct) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    out[idx] = up16(in[(size_t)(idx / ct) * C + (int)(idx % ct)]);
}

#if MAPDIT_DT == 0
// ---- fp32 / byte / fp64 kernels: built once (no _f16 twin) -------------------------------------------------------------------------
// Bilinear resize to S x S with align_corners = False and no antialiasing, F.interpolate's map: source coordinate
// (dst + 0.5) * in / out - 0.5 clamped at 0; i0 = floor, i1 = i0 + 1 clamped to the last pixel, weights (1 - l, l); the row blend of
// the two column blends.  u8 != 0: img is uint8 [N, H, W, C] and each tap is taken to [-1, 1] first, v / 255 * 2 - 1 (the blend's
// weights sum to 1, so this is the blend of the bytes mapped afterwards, with the fp32 rounding on values <= 1 instead of <= 255);
// else img is fp32 [N, C, H, W] already in [-1, 1].  out fp32 NHWC [N, S, S, C].
__global__ __launch_bounds__(256) void inc_resize_kernel(const void* __restrict__ img, int u8, float* __restrict__ out, long total, int H, int W,
                                                         int C, int S) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long pix = idx / C;
    const int x = (int)(pix % S);
    const long row = pix / S;
    const int y = (int)(row % S);
    const long n = row / S;
    // source coordinate (2 d + 1) in / (2 S) - 1/2 = ((2 d + 1) in - S) / (2 S): the numerator is an exact integer, so the floor and the
    // remainder are exact and the weight is one fp32 division of two small integers
    long ny = (long)(2 * y + 1) * H - S, nx = (long)(2 * x + 1) * W - S;
    ny = ny < 0 ? 0 : ny;
    nx = nx < 0 ? 0 : nx;
    int y0 = (int)(ny / (2 * S)), x0 = (int)(nx / (2 * S));
    float ly = (float)(ny - (long)y0 * 2 * S) / (float)(2 * S), lx = (float)(nx - (long)x0 * 2 * S) / (float)(2 * S);
    if (y0 >= H - 1) {
        y0 = H - 1;
        ly = 0.f;
    }
    if (x0 >= W - 1) {
        x0 = W - 1;
        lx = 0.f;
    }
    const int y1 = y0 < H - 1 ? y0 + 1 : y0, x1 = x0 < W - 1 ? x0 + 1 : x0;
    const float hy = 1.f - ly, hx = 1.f - lx;
    float v00, v01, v10, v11;
    if (u8) {
        const uint8_t* b = (const uint8_t*)img + (size_t)n * H * W * C + c;
        v00 = (float)b[((size_t)y0 * W + x0) * C] / 255.f * 2.f - 1.f;
        v01 = (float)b[((size_t)y0 * W + x1) * C] / 255.f * 2.f - 1.f;
        v10 = (float)b[((size_t)y1 * W + x0) * C] / 255.f * 2.f - 1.f;
        v11 = (float)b[((size_t)y1 * W + x1) * C] / 255.f * 2.f - 1.f;
    } else {
        const float* b = (const float*)img + ((size_t)n * C + c) * H * W;
        v00 = b[(size_t)y0 * W + x0];
        v01 = b[(size_t)y0 * W + x1];
        v10 = b[(size_t)y1 * W + x0];
        v11 = b[(size_t)y1 * W + x1];
    }
    out[idx] = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// Feature statistics in fp64: sum[d] += sum_n x[n][d], outer[i][j] += sum_n x[n][i] * x[n][j].  One thread per output element walks
// the samples in index order and adds to the value it read: no atomics, no partial sums - the result is a function of the sequence
// of samples, not of the batches it arrives in.  (The product of two fp32 values is exact in fp64.)
__global__ __launch_bounds__(256) void inc_stats_outer_kernel(const float* __restrict__ x, int N, int D, double* __restrict__ outer) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= D || j >= D) return;
    double a = outer[(size_t)i * D + j];
    for (int n = 0; n < N; ++n) a += (double)x[(size_t)n * D + i] * (double)x[(size_t)n * D + j];
    outer[(size_t)i * D + j] = a;
}

__global__ __launch_bounds__(256) void inc_stats_sum_kernel(const float* __restrict__ x, int N, int D, double* __restrict__ sum) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double a = sum[d];
    for (int n = 0; n < N; ++n) a += (double)x[(size_t)n * D + d];
    sum[d] = a;
}
#endif

MD_NS_CLOSE

// ---- entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int MD_SYM(inc_conv)(const mapdit_inc_conv_t* a, void* stream) {
    MD_CHECK(a && a->in && a->w && a->bias && a->out, "inc_conv: null argument");
    MD_CHECK(a->N > 0 && a->Hin > 0 && a->Win > 0 && a->Cin > 0 && a->Cout > 0, "inc_conv: empty shape N=%d Hin=%d Win=%d Cin=%d Cout=%d", a->N,
             a->Hin, a->Win, a->Cin, a->Cout);
    MD_CHECK(a->kh >= 1 && a->kh <= 7 && a->kw >= 1 && a->kw <= 7, "inc_conv: kernel of %d x %d (1..7 each way)", a->kh, a->kw);
    MD_CHECK(a->stride == 1 || a->stride == 2, "inc_conv: stride=%d (1 or 2)", a->stride);
    MD_CHECK(a->pad_h >= 0 && a->pad_h < a->kh && a->pad_w >= 0 && a->pad_w < a->kw, "inc_conv: pad (%d, %d) for a %d x %d kernel", a->pad_h, a->pad_w,
             a->kh, a->kw);
    MD_CHECK(a->in_kind == MAPDIT_INC_IN_16 || a->in_kind == MAPDIT_INC_IN_F32, "inc_conv: bad in_kind %d", a->in_kind);
    MD_CHECK(a->out_kind == MAPDIT_INC_OUT_F32 || a->out_kind == MAPDIT_INC_OUT_16, "inc_conv: bad out_kind %d", a->out_kind);
    MD_CHECK(a->Hin + 2 * a->pad_h >= a->kh && a->Win + 2 * a->pad_w >= a->kw, "inc_conv: a %d x %d kernel does not fit a %d x %d input", a->kh, a->kw,
             a->Hin, a->Win);
    MD_CHECK(a->c_off >= 0 && a->ld_out >= a->c_off + a->Cout, "inc_conv: channels [%d, %d) do not fit rows of ld_out=%d", a->c_off, a->c_off + a->Cout,
             a->ld_out);
    const int Ho = (a->Hin + 2 * a->pad_h - a->kh) / a->stride + 1, Wo = (a->Win + 2 * a->pad_w - a->kw) / a->stride + 1;
    const long M = (long)a->N * Ho * Wo;
    MD_CHECK(M < (1L << 31) && (long)a->N * a->Hin * a->Win < (1L << 31) && M * a->ld_out < (1L << 40), "inc_conv: %ld output pixels are too many", M);
    const long Ktot = (long)a->kh * a->kw * a->Cin;
    MD_CHECK(Ktot < (1L << 24), "inc_conv: K = %ld is too long", Ktot);
    // stride and padding as given, the extent and the source are the input; the kinds share the VAE's values but for the 16-bit store
    const md_conv_t p{a->in, (const bf16_t*)a->w, a->bias, nullptr, a->out, a->in_kind, a->out_kind == MAPDIT_INC_OUT_16 ? MAPDIT_VAE_OUT_16 : MAPDIT_VAE_OUT_F32,
                      a->Hin, a->Win, a->Hin, a->Win, 0, a->kh, a->kw, a->stride, a->pad_h, a->pad_w, Ho, Wo, a->Cin, a->Cout, (int)Ktot, M,
                      a->ld_out, a->c_off, a->relu ? 1 : 0};
    const bool aligned = !(((uintptr_t)a->in | (uintptr_t)a->w) & 15);
    const bool mfma = a->in_kind == MAPDIT_INC_IN_16 && a->Cin % 16 == 0 && a->Cout % 16 == 0 && aligned;
    return MD_SYM(conv_launch)("inc_conv", &p, mfma ? MD_CONV_64 : MD_CONV_PLAIN, stream);
}

extern "C" int MD_SYM(inc_pool)(const void* in, int in_kind, void* out, int out_kind, int N, int H, int W, int C, int mode, int ld_out, int c_off,
                                void* stream) {
    MD_CHECK(in && out, "inc_pool: null argument");
    MD_CHECK(N > 0 && H > 0 && W > 0 && C > 0, "inc_pool: N=%d, H=%d, W=%d, C=%d must be positive", N, H, W, C);
    MD_CHECK(mode == MAPDIT_INC_POOL_MAX_S2 || mode == MAPDIT_INC_POOL_AVG || mode == MAPDIT_INC_POOL_MAX_S1, "inc_pool: bad mode %d", mode);
    MD_CHECK(in_kind == MAPDIT_INC_IN_16 || in_kind == MAPDIT_INC_IN_F32, "inc_pool: bad in_kind %d", in_kind);
    MD_CHECK(out_kind == MAPDIT_INC_OUT_F32 || out_kind == MAPDIT_INC_OUT_16, "inc_pool: bad out_kind %d", out_kind);
    MD_CHECK(mode != MAPDIT_INC_POOL_MAX_S2 || (H >= 3 && W >= 3), "inc_pool: a %d x %d image is smaller than the 3 x 3 window", H, W);
    MD_CHECK(c_off >= 0 && ld_out >= c_off + C, "inc_pool: channels [%d, %d) do not fit rows of ld_out=%d", c_off, c_off + C, ld_out);
    const int Ho = mode == MAPDIT_INC_POOL_MAX_S2 ? (H - 3) / 2 + 1 : H, Wo = mode == MAPDIT_INC_POOL_MAX_S2 ? (W - 3) / 2 + 1 : W;
    const long total = (long)N * Ho * Wo * C;
    MD_CHECK((long)N * H * W < (1L << 31) && total < (1L << 38) && (long)N * Ho * Wo * ld_out < (1L << 40), "inc_pool: %ld elements are too many", total);
    inc_pool_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(in, in_kind == MAPDIT_INC_IN_F32, out, out_kind == MAPDIT_INC_OUT_16, total, H, W,
                                                                      C, Ho, Wo, mode, ld_out, c_off);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(inc_global_avg)(const void* in, int in_kind, float* out, int N, int HW, int C, void* stream) {
    MD_CHECK(in && out, "inc_global_avg: null argument");
    MD_CHECK(N > 0 && HW > 0 && C > 0, "inc_global_avg: N=%d, HW=%d, C=%d must be positive", N, HW, C);
    MD_CHECK(in_kind == MAPDIT_INC_IN_16 || in_kind == MAPDIT_INC_IN_F32, "inc_global_avg: bad in_kind %d", in_kind);
    const long total = (long)N * C;
    MD_CHECK(total < (1L << 31) && total * HW < (1L << 40), "inc_global_avg: %ld x %d elements are too many", total, HW);
    inc_global_avg_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(in, in_kind == MAPDIT_INC_IN_F32, out, total, HW, C);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

#if MAPDIT_DT == 0
static int inc_resize_launch(const char* who, const void* img, int u8, float* out, int N, int H, int W, int C, int S, void* stream) {
    MD_CHECK(img && out, "%s: null argument", who);
    MD_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && S > 0, "%s: N=%d, H=%d, W=%d, C=%d, size=%d must be positive", who, N, H, W, C, S);
    MD_CHECK(H < (1 << 24) && W < (1 << 24) && S < (1 << 22), "%s: H=%d, W=%d (below 2^24) or size=%d (below 2^22) is too large", who, H, W, S);
    const long total = (long)N * S * S * C;
    MD_CHECK(total < (1L << 38) && (long)N * H * W * C < (1L << 40), "%s: %ld elements are too many for one call", who, total);
    inc_resize_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(img, u8, out, total, H, W, C, S);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_inc_resize_u8(const uint8_t* img, float* out, int N, int H, int W, int C, int size, void* stream) {
    return inc_resize_launch("inc_resize_u8", img, 1, out, N, H, W, C, size, stream);
}

extern "C" int mapdit_inc_resize_f32(const float* img, float* out, int N, int H, int W, int C, int size, void* stream) {
    return inc_resize_launch("inc_resize_f32", img, 0, out, N, H, W, C, size, stream);
}

extern "C" int mapdit_inc_stats_accumulate(const float* feat, int N, int D, double* sum, double* outer, void* stream) {
    MD_CHECK(feat && sum && outer, "inc_stats_accumulate: null argument");
    MD_CHECK(N > 0 && D > 0 && D <= 65536, "inc_stats_accumulate: N=%d and D=%d must be positive (D <= 65536)", N, D);
    MD_CHECK(!(((uintptr_t)sum | (uintptr_t)outer) & 7), "inc_stats_accumulate: sum and outer must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    inc_stats_sum_kernel<<<cdiv(D, 256), 256, 0, st>>>(feat, N, D, sum);
    const dim3 grid((unsigned)cdiv(D, 64), (unsigned)cdiv(D, 4));
    inc_stats_outer_kernel<<<grid, 256, 0, st>>>(feat, N, D, outer);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
#endif

// ---- the network -------------------------------------------------------------------------------------------------------------------
// One walk serves the three uses: `shape` (no launches; records every convolution's shape and the largest activation), the
// workspace query and the run.  Buffers: X the block's input, Y its concatenated output (each branch's last convolution, and the
// max-pool branches of Mixed_6a / 7a, write their channel slice of it), T1 / T2 the branches' temporaries; all 16-bit NHWC of maxE
// elements.  IMG: the fp32 image at size x size; FIN: the last block's fp32 output.
namespace {
struct IncLayer {
    int cin, cout, kh, kw, st;
};

struct IncWalk {
    bool dry;
    int N;
    void* stream;
    const void* const* wt;
    uint16_t *X, *Y, *T1, *T2;
    float *IMG, *FIN;
    float* TAP;                  // the spatial tap's destination [N, tapH * tapW * MAPDIT_INC_SPATIAL_CHANNELS], or null: no tap
    int tapH, tapW;
    int li;                      // the next convolution's number in execution order
    size_t maxE, finE;
    IncLayer layers[MAPDIT_INC_NUM_CONV];

    void note(int H, int W, int C) {
        const size_t e = (size_t)N * H * W * C;
        maxE = e > maxE ? e : maxE;
    }
    int conv(const void* in, int in_kind, int H, int W, int cin, int cout, int kh, int kw, int st, int ph, int pw, void* out, int out_kind, int ld,
             int coff, int* Ho, int* Wo) {
        MD_CHECK(li < MAPDIT_INC_NUM_CONV, "inception: more than %d convolutions", MAPDIT_INC_NUM_CONV);
        MD_CHECK(H + 2 * ph >= kh && W + 2 * pw >= kw, "inception: the image size is too small: convolution %d (%d x %d) meets a %d x %d input", li, kh,
                 kw, H, W);
        const int ho = (H + 2 * ph - kh) / st + 1, wo = (W + 2 * pw - kw) / st + 1;
        layers[li] = IncLayer{cin, cout, kh, kw, st};
        const int i = li++;
        if (Ho) *Ho = ho;
        if (Wo) *Wo = wo;
        if (out_kind == MAPDIT_INC_OUT_16) note(ho, wo, ld);
        else finE = (size_t)N * ho * wo * ld;
        if (dry) return MAPDIT_OK;
        const mapdit_inc_conv_t a{in, in_kind, (const uint16_t*)wt[2 * i], (const float*)wt[2 * i + 1], out, out_kind, N, H, W, cin, cout, kh, kw, st, ph,
                                  pw, 1, ld, coff};
        return MD_SYM(inc_conv)(&a, stream);
    }
    // 16-bit [N, H, W, cin] -> 16-bit, the common case
    int c16(const uint16_t* in, int H, int W, int cin, int cout, int kh, int kw, int st, int ph, int pw, uint16_t* out, int ld, int coff) {
        return conv(in, MAPDIT_INC_IN_16, H, W, cin, cout, kh, kw, st, ph, pw, out, MAPDIT_INC_OUT_16, ld, coff, nullptr, nullptr);
    }
    int pool(const uint16_t* in, int H, int W, int C, int mode, uint16_t* out, int ld, int coff) {
        MD_CHECK(mode != MAPDIT_INC_POOL_MAX_S2 || (H >= 3 && W >= 3), "inception: the image size is too small: a stride-2 pool meets a %d x %d input", H, W);
        const int ho = mode == MAPDIT_INC_POOL_MAX_S2 ? (H - 3) / 2 + 1 : H, wo = mode == MAPDIT_INC_POOL_MAX_S2 ? (W - 3) / 2 + 1 : W;
        note(ho, wo, ld);
        if (dry) return MAPDIT_OK;
        return MD_SYM(inc_pool)(in, MAPDIT_INC_IN_16, out, MAPDIT_INC_OUT_16, N, H, W, C, mode, ld, coff, stream);
    }
    void swap_xy() {
        uint16_t* t = X;
        X = Y;
        Y = t;
    }
    // after Mixed_6d: X is the block's concatenated [N, H, W, 768] output, channels [0, 192) of it the branch1x1 unit
    int tap(int H, int W) {
        tapH = H;
        tapW = W;
        if (dry || !TAP) return MAPDIT_OK;
        const long total = (long)N * H * W * MAPDIT_INC_SPATIAL_CHANNELS;
        inc_tap_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)X, TAP, total, 768, MAPDIT_INC_SPATIAL_CHANNELS);
        MD_LAUNCH_CHECK();
        return MAPDIT_OK;
    }

    // Mixed_5b / 5c / 5d
    int block_a(int H, int W, int cin, int pw_) {
        const int ld = 224 + pw_;
        MD_TRY(c16(X, H, W, cin, 64, 1, 1, 1, 0, 0, Y, ld, 0));
        MD_TRY(c16(X, H, W, cin, 48, 1, 1, 1, 0, 0, T1, 48, 0));
        MD_TRY(c16(T1, H, W, 48, 64, 5, 5, 1, 2, 2, Y, ld, 64));
        MD_TRY(c16(X, H, W, cin, 64, 1, 1, 1, 0, 0, T1, 64, 0));
        MD_TRY(c16(T1, H, W, 64, 96, 3, 3, 1, 1, 1, T2, 96, 0));
        MD_TRY(c16(T2, H, W, 96, 96, 3, 3, 1, 1, 1, Y, ld, 128));
        MD_TRY(pool(X, H, W, cin, MAPDIT_INC_POOL_AVG, T1, cin, 0));
        MD_TRY(c16(T1, H, W, cin, pw_, 1, 1, 1, 0, 0, Y, ld, 224));
        swap_xy();
        return MAPDIT_OK;
    }
    // Mixed_6a: 288 -> 768, the size halves
    int block_b(int* H, int* W) {
        const int h = *H, w = *W, cin = 288, ld = 768;
        MD_CHECK(h >= 3 && w >= 3, "inception: the image size is too small: Mixed_6a meets a %d x %d input", h, w);
        MD_TRY(c16(X, h, w, cin, 384, 3, 3, 2, 0, 0, Y, ld, 0));
        MD_TRY(c16(X, h, w, cin, 64, 1, 1, 1, 0, 0, T1, 64, 0));
        MD_TRY(c16(T1, h, w, 64, 96, 3, 3, 1, 1, 1, T2, 96, 0));
        MD_TRY(c16(T2, h, w, 96, 96, 3, 3, 2, 0, 0, Y, ld, 384));
        MD_TRY(pool(X, h, w, cin, MAPDIT_INC_POOL_MAX_S2, Y, ld, 480));
        *H = (h - 3) / 2 + 1;
        *W = (w - 3) / 2 + 1;
        swap_xy();
        return MAPDIT_OK;
    }
    // Mixed_6b .. 6e
    int block_c(int H, int W, int c7) {
        const int cin = 768, ld = 768;
        MD_TRY(c16(X, H, W, cin, 192, 1, 1, 1, 0, 0, Y, ld, 0));
        MD_TRY(c16(X, H, W, cin, c7, 1, 1, 1, 0, 0, T1, c7, 0));
        MD_TRY(c16(T1, H, W, c7, c7, 1, 7, 1, 0, 3, T2, c7, 0));
        MD_TRY(c16(T2, H, W, c7, 192, 7, 1, 1, 3, 0, Y, ld, 192));
        MD_TRY(c16(X, H, W, cin, c7, 1, 1, 1, 0, 0, T1, c7, 0));
        MD_TRY(c16(T1, H, W, c7, c7, 7, 1, 1, 3, 0, T2, c7, 0));
        MD_TRY(c16(T2, H, W, c7, c7, 1, 7, 1, 0, 3, T1, c7, 0));
        MD_TRY(c16(T1, H, W, c7, c7, 7, 1, 1, 3, 0, T2, c7, 0));
        MD_TRY(c16(T2, H, W, c7, 192, 1, 7, 1, 0, 3, Y, ld, 384));
        MD_TRY(pool(X, H, W, cin, MAPDIT_INC_POOL_AVG, T1, cin, 0));
        MD_TRY(c16(T1, H, W, cin, 192, 1, 1, 1, 0, 0, Y, ld, 576));
        swap_xy();
        return MAPDIT_OK;
    }
    // Mixed_7a: 768 -> 1280, the size halves
    int block_d(int* H, int* W) {
        const int h = *H, w = *W, cin = 768, ld = 1280;
        MD_CHECK(h >= 3 && w >= 3, "inception: the image size is too small: Mixed_7a meets a %d x %d input", h, w);
        MD_TRY(c16(X, h, w, cin, 192, 1, 1, 1, 0, 0, T1, 192, 0));
        MD_TRY(c16(T1, h, w, 192, 320, 3, 3, 2, 0, 0, Y, ld, 0));
        MD_TRY(c16(X, h, w, cin, 192, 1, 1, 1, 0, 0, T1, 192, 0));
        MD_TRY(c16(T1, h, w, 192, 192, 1, 7, 1, 0, 3, T2, 192, 0));
        MD_TRY(c16(T2, h, w, 192, 192, 7, 1, 1, 3, 0, T1, 192, 0));
        MD_TRY(c16(T1, h, w, 192, 192, 3, 3, 2, 0, 0, Y, ld, 320));
        MD_TRY(pool(X, h, w, cin, MAPDIT_INC_POOL_MAX_S2, Y, ld, 512));
        *H = (h - 3) / 2 + 1;
        *W = (w - 3) / 2 + 1;
        swap_xy();
        return MAPDIT_OK;
    }
    // Mixed_7b (average pool, 16-bit output into Y) / Mixed_7c (the port's 3 x 3 max pool, fp32 output into FIN)
    int block_e(int H, int W, int cin, int pool_mode, bool last) {
        const int ld = 2048, ok = last ? MAPDIT_INC_OUT_F32 : MAPDIT_INC_OUT_16;
        void* O = last ? (void*)FIN : (void*)Y;
        const int k16 = MAPDIT_INC_IN_16;
        MD_TRY(conv(X, k16, H, W, cin, 320, 1, 1, 1, 0, 0, O, ok, ld, 0, nullptr, nullptr));
        MD_TRY(c16(X, H, W, cin, 384, 1, 1, 1, 0, 0, T1, 384, 0));
        MD_TRY(conv(T1, k16, H, W, 384, 384, 1, 3, 1, 0, 1, O, ok, ld, 320, nullptr, nullptr));
        MD_TRY(conv(T1, k16, H, W, 384, 384, 3, 1, 1, 1, 0, O, ok, ld, 704, nullptr, nullptr));
        MD_TRY(c16(X, H, W, cin, 448, 1, 1, 1, 0, 0, T1, 448, 0));
        MD_TRY(c16(T1, H, W, 448, 384, 3, 3, 1, 1, 1, T2, 384, 0));
        MD_TRY(conv(T2, k16, H, W, 384, 384, 1, 3, 1, 0, 1, O, ok, ld, 1088, nullptr, nullptr));
        MD_TRY(conv(T2, k16, H, W, 384, 384, 3, 1, 1, 1, 0, O, ok, ld, 1472, nullptr, nullptr));
        MD_TRY(pool(X, H, W, cin, pool_mode, T1, cin, 0));
        MD_TRY(conv(T1, k16, H, W, cin, 192, 1, 1, 1, 0, 0, O, ok, ld, 1856, nullptr, nullptr));
        if (!last) swap_xy();
        return MAPDIT_OK;
    }

    // IMG [N, S, S, 3] -> FIN [N, Hf, Wf, 2048]
    int run(int S, int* Hf, int* Wf) {
        int H = S, W = S;
        li = 0;
        maxE = finE = 0;
        MD_TRY(conv(IMG, MAPDIT_INC_IN_F32, H, W, 3, 32, 3, 3, 2, 0, 0, X, MAPDIT_INC_OUT_16, 32, 0, &H, &W));        // Conv2d_1a_3x3
        MD_TRY(conv(X, MAPDIT_INC_IN_16, H, W, 32, 32, 3, 3, 1, 0, 0, Y, MAPDIT_INC_OUT_16, 32, 0, &H, &W));          // Conv2d_2a_3x3
        MD_TRY(c16(Y, H, W, 32, 64, 3, 3, 1, 1, 1, X, 64, 0));                                                        // Conv2d_2b_3x3
        MD_TRY(pool(X, H, W, 64, MAPDIT_INC_POOL_MAX_S2, Y, 64, 0));
        H = (H - 3) / 2 + 1;
        W = (W - 3) / 2 + 1;
        MD_TRY(c16(Y, H, W, 64, 80, 1, 1, 1, 0, 0, X, 80, 0));                                                        // Conv2d_3b_1x1
        MD_TRY(conv(X, MAPDIT_INC_IN_16, H, W, 80, 192, 3, 3, 1, 0, 0, Y, MAPDIT_INC_OUT_16, 192, 0, &H, &W));        // Conv2d_4a_3x3
        MD_TRY(pool(Y, H, W, 192, MAPDIT_INC_POOL_MAX_S2, X, 192, 0));
        H = (H - 3) / 2 + 1;
        W = (W - 3) / 2 + 1;
        MD_TRY(block_a(H, W, 192, 32));
        MD_TRY(block_a(H, W, 256, 64));
        MD_TRY(block_a(H, W, 288, 64));
        MD_TRY(block_b(&H, &W));
        MD_TRY(block_c(H, W, 128));
        MD_TRY(block_c(H, W, 160));
        MD_TRY(block_c(H, W, 160));
        MD_TRY(tap(H, W));                                                                                            // Mixed_6d
        MD_TRY(block_c(H, W, 192));
        MD_TRY(block_d(&H, &W));
        MD_TRY(block_e(H, W, 1280, MAPDIT_INC_POOL_AVG, false));
        MD_TRY(block_e(H, W, 2048, MAPDIT_INC_POOL_MAX_S1, true));
        MD_CHECK(li == MAPDIT_INC_NUM_CONV, "inception: %d convolutions walked, %d declared", li, MAPDIT_INC_NUM_CONV);
        *Hf = H;
        *Wf = W;
        return MAPDIT_OK;
    }
};

struct IncPlan {
    size_t off_img, off_fin, off_x, off_y, off_t1, off_t2, total;
    int Hf, Wf;
};

int inc_plan(const mapdit_inc_config_t* cfg, int N, IncWalk* wk, IncPlan* pl) {
    MD_CHECK(cfg, "inception: null config");
    MD_CHECK(N > 0, "inception: N=%d must be positive", N);
    MD_CHECK(cfg->image_size >= 75 && cfg->image_size <= 4096, "inception: image_size=%d (75 .. 4096; FID uses 299)", cfg->image_size);
    MD_CHECK((long)N * cfg->image_size * cfg->image_size < (1L << 31), "inception: N=%d images of %d x %d are too many pixels for one call", N,
             cfg->image_size, cfg->image_size);
    *wk = IncWalk{};
    wk->dry = true;
    wk->N = N;
    MD_TRY(wk->run(cfg->image_size, &pl->Hf, &pl->Wf));
    size_t o = 0;
    pl->off_img = o; o += md_up256((size_t)N * cfg->image_size * cfg->image_size * 3 * 4);
    pl->off_fin = o; o += md_up256(wk->finE * 4);
    pl->off_x = o; o += md_up256(wk->maxE * 2);
    pl->off_y = o; o += md_up256(wk->maxE * 2);
    pl->off_t1 = o; o += md_up256(wk->maxE * 2);
    pl->off_t2 = o; o += md_up256(wk->maxE * 2);
    pl->total = o;
    return MAPDIT_OK;
}
}  // namespace

#if MAPDIT_DT == 0
extern "C" size_t mapdit_inc_workspace_bytes(const mapdit_inc_config_t* cfg, int N) {
    IncWalk wk;
    IncPlan pl;
    return inc_plan(cfg, N, &wk, &pl) == MAPDIT_OK ? pl.total : 0;
}

extern "C" int mapdit_inc_layer_shape(int index, int* cin, int* cout, int* kh, int* kw, int* stride) {
    MD_CHECK(index >= 0 && index < MAPDIT_INC_NUM_CONV, "inc_layer_shape: index %d outside [0, %d)", index, MAPDIT_INC_NUM_CONV);
    MD_CHECK(cin && cout && kh && kw && stride, "inc_layer_shape: null argument");
    const mapdit_inc_config_t cfg{299};
    IncWalk wk;
    IncPlan pl;
    MD_TRY(inc_plan(&cfg, 1, &wk, &pl));
    const IncLayer& l = wk.layers[index];
    *cin = l.cin;
    *cout = l.cout;
    *kh = l.kh;
    *kw = l.kw;
    *stride = l.st;
    return MAPDIT_OK;
}

extern "C" int mapdit_inc_spatial_shape(const mapdit_inc_config_t* cfg, int* hs, int* ws, int* channels) {
    MD_CHECK(hs && ws && channels, "inc_spatial_shape: null argument");
    IncWalk wk;
    IncPlan pl;
    MD_TRY(inc_plan(cfg, 1, &wk, &pl));
    *hs = wk.tapH;
    *ws = wk.tapW;
    *channels = MAPDIT_INC_SPATIAL_CHANNELS;
    return MAPDIT_OK;
}
#endif

// the one run: `spatial` null is mapdit_inc_features (no tap kernel, the same launches as ever)
static int inc_features_run(const char* who, const mapdit_inc_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H,
                            int W, float* feat, float* spatial, void* workspace, size_t ws_bytes, void* stream) {
    IncWalk wk;
    IncPlan pl;
    MD_TRY(inc_plan(cfg, N, &wk, &pl));
    MD_CHECK(wt && images && feat && workspace, "%s: null argument", who);
    MD_CHECK(img_kind == MAPDIT_INC_IMG_U8_NHWC || img_kind == MAPDIT_INC_IMG_F32_NCHW, "%s: bad img_kind %d", who, img_kind);
    MD_CHECK(H >= 8 && W >= 8, "%s: images of %d x %d (8 x 8 at the least)", who, H, W);
    MD_CHECK(ws_bytes >= pl.total, "%s: workspace of %zu bytes, %zu needed (mapdit_inc_workspace_bytes)", who, ws_bytes, pl.total);
    MD_CHECK(!((uintptr_t)workspace & 255), "%s: the workspace must be 256-byte aligned", who);
    MD_CHECK(!((uintptr_t)spatial & 3), "%s: spatial is not 4-byte aligned", who);
    for (int i = 0; i < 2 * MAPDIT_INC_NUM_CONV; ++i) MD_CHECK(wt[i], "%s: weight slot %d is null", who, i);
    char* ws = (char*)workspace;
    wk = IncWalk{};
    wk.dry = false;
    wk.N = N;
    wk.stream = stream;
    wk.wt = wt;
    wk.TAP = spatial;
    wk.IMG = (float*)(ws + pl.off_img);
    wk.FIN = (float*)(ws + pl.off_fin);
    wk.X = (uint16_t*)(ws + pl.off_x);
    wk.Y = (uint16_t*)(ws + pl.off_y);
    wk.T1 = (uint16_t*)(ws + pl.off_t1);
    wk.T2 = (uint16_t*)(ws + pl.off_t2);
    const int S = cfg->image_size;
    if (img_kind == MAPDIT_INC_IMG_U8_NHWC) MD_TRY(mapdit_inc_resize_u8((const uint8_t*)images, wk.IMG, N, H, W, 3, S, stream));
    else MD_TRY(mapdit_inc_resize_f32((const float*)images, wk.IMG, N, H, W, 3, S, stream));
    int Hf = 0, Wf = 0;
    MD_TRY(wk.run(S, &Hf, &Wf));
    return MD_SYM(inc_global_avg)(wk.FIN, MAPDIT_INC_IN_F32, feat, N, Hf * Wf, 2048, stream);
}

extern "C" int MD_SYM(inc_features)(const mapdit_inc_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H, int W,
                                    float* feat, void* workspace, size_t ws_bytes, void* stream) {
    return inc_features_run("inc_features", cfg, wt, images, img_kind, N, H, W, feat, nullptr, workspace, ws_bytes, stream);
}

extern "C" int MD_SYM(inc_features_tap)(const mapdit_inc_config_t* cfg, const void* const* wt, const void* images, int img_kind, int N, int H,
                                        int W, float* feat, float* spatial, void* workspace, size_t ws_bytes, void* stream) {
    return inc_features_run("inc_features_tap", cfg, wt, images, img_kind, N, H, W, feat, spatial, workspace, ws_bytes, stream);
}
