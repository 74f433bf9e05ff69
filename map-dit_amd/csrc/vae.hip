// VAE (AutoencoderKL layout), both directions: GroupNorm(+SiLU) over NHWC, a row softmax, the encoder's pointwise kernels (image
// preparation, posterior head, latent statistics), the convolution entry points and the two host plans that sequence a decode or an
// encode on one stream (mapdit.h, "VAE").  Built once per 16-bit operand format (csrc/Makefile).
//
// Convolution: conv.hip's kernels behind one coordinate map (common.h, md_conv_t).  "Same" convolution: st = 1, pad = k / 2, extent =
// the output size.  up2: the extent is the upsampled size, the source half of it.  Stride-2 downsample (F.pad(x, (0, 1, 0, 1)) + a 3 x 3
// convolution of stride 2 without padding): st = 2, pad = 0, extent = source = (Hin, Win) - the pad row and column are the taps at
// 2 y + ky == Hin, 2 x + kx == Win, zeros that are never loaded; nothing is added at the top or left.
#include "common.h"

MD_NS_OPEN

// ---- GroupNorm (+ SiLU) over NHWC -----------------------------------------------------------------------------------------------
// One workgroup per (sample, group).  Statistics in ONE pass over d = x - x[first element of the group] with fp64 sums of d and d * d
// (the shift keeps d small for channels with a large mean; fp64 keeps the sum of squares exact far beyond what the bounds ask), added
// in a fixed order: thread (pixel stride 256), wave (xor shuffles), the four waves through LDS.  The second pass normalises in fp32.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void vae_groupnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, int silu, bf16_t* __restrict__ out,
                                                          float* __restrict__ stats, int HW, int C, int G) {
    __shared__ double red[2][4];
    __shared__ float ms[2];
    const int n = blockIdx.x / G, g = blockIdx.x % G, cpg = C / G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)n * HW * C + (size_t)g * cpg;
    const float* xb = x + base;
    const float shift = xb[0];
    double s = 0.0, ss = 0.0;
    for (int px = tid; px < HW; px += 256) {
        const float* xp = xb + (size_t)px * C;
        for (int c = 0; c < cpg; ++c) {
            const double d = (double)(xp[c] - shift);
            s += d;
            ss += d * d;
        }
    }
    s = wave_sum_d(s);
    ss = wave_sum_d(ss);
    if (lane == 0) {
        red[0][wave] = s;
        red[1][wave] = ss;
    }
    __syncthreads();
    if (tid == 0) {
        const double cnt = (double)HW * cpg;
        const double sd = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double sq = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        const double md = sd / cnt;
        double var = sq / cnt - md * md;
        var = var > 0.0 ? var : 0.0;
        const float mean = (float)((double)shift + md), rstd = (float)(1.0 / sqrt(var + (double)eps));
        ms[0] = mean;
        ms[1] = rstd;
        if (stats) {
            stats[((size_t)n * G + g) * 2] = mean;
            stats[((size_t)n * G + g) * 2 + 1] = rstd;
        }
    }
    __syncthreads();
    const float mean = ms[0], rstd = ms[1];
    bf16_t* ob = out + base;
    for (int px = tid; px < HW; px += 256) {
        const float* xp = xb + (size_t)px * C;
        bf16_t* op = ob + (size_t)px * C;
        for (int c = 0; c < cpg; ++c) {
            float v = (xp[c] - mean) * rstd * gamma[g * cpg + c] + beta[g * cpg + c];
            if (silu) v = v / (1.f + __expf(-v));
            op[c] = cvt16s(v);
        }
    }
}

// The split form, for tensors large enough to matter (one workgroup per (sample, group) reads 4 * C/G bytes of every C * 4-byte pixel
// row: an eighth of each cache line at C = 128, and N * G workgroups in all).  Both stages read whole pixel rows: thread = (pixel lane,
// four adjacent channels), 256 / (C / 4) pixel lanes.  Stage 1: a workgroup owns GN_PX pixels of one sample and writes, per group, its
// fp64 sums of d and d * d (d = x - the group's first element of the sample, as above) - thread, then the workgroup through LDS in
// (pixel lane, channel) order.  Stage 2: every workgroup adds the partials of its sample in chunk order (the same few KB for all of
// them), then normalises its own GN_PX pixels.  No atomics; a sample's statistics do not depend on the batch it is in.
constexpr int GN_PX = 1024;

__global__ __launch_bounds__(256) void vae_gn_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int HW, int C, int G) {
    __shared__ double ls[2][1024];                        // [pixel lane][channel]: 256 / (C / 4) * C = 1024 entries
    const int tid = threadIdx.x, cols = C >> 2, col = tid % cols, pl = tid / cols, lanes = 256 / cols, cpg = C / G;
    const int chunk = blockIdx.x, n = blockIdx.y;
    const float* xb = x + (size_t)n * HW * C;
    float sh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[e] = xb[((col * 4 + e) / cpg) * cpg];
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
    const int p0 = chunk * GN_PX, p1 = p0 + GN_PX < HW ? p0 + GN_PX : HW;
    for (int px = p0 + pl; px < p1; px += lanes) {
        const float4 v = *(const float4*)(xb + (size_t)px * C + col * 4);
        const float ve[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)(ve[e] - sh[e]);
            s[e] += d;
            ss[e] += d * d;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        ls[0][pl * C + col * 4 + e] = s[e];
        ls[1][pl * C + col * 4 + e] = ss[e];
    }
    __syncthreads();
    if (tid < G) {
        double a = 0.0, b = 0.0;
        for (int l = 0; l < lanes; ++l)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
                a += ls[0][l * C + c];
                b += ls[1][l * C + c];
            }
        double* o = part + (((size_t)n * gridDim.x + chunk) * G + tid) * 2;
        o[0] = a;
        o[1] = b;
    }
}

__global__ __launch_bounds__(256) void vae_gn_apply_kernel(const float* __restrict__ x, const double* __restrict__ part,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int silu,
                                                         bf16_t* __restrict__ out, float* __restrict__ stats, int HW, int C, int G) {
    __shared__ float ms[2][256];
    const int tid = threadIdx.x, cols = C >> 2, col = tid % cols, pl = tid / cols, lanes = 256 / cols, cpg = C / G;
    const int chunk = blockIdx.x, n = blockIdx.y, nchunks = gridDim.x;
    const float* xb = x + (size_t)n * HW * C;
    if (tid < G) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < nchunks; ++k) {
            const double* pp = part + (((size_t)n * nchunks + k) * G + tid) * 2;
            a += pp[0];
            b += pp[1];
        }
        const double cnt = (double)HW * cpg, md = a / cnt;
        double var = b / cnt - md * md;
        var = var > 0.0 ? var : 0.0;
        const float mean = (float)((double)xb[tid * cpg] + md), rstd = (float)(1.0 / sqrt(var + (double)eps));
        ms[0][tid] = mean;
        ms[1][tid] = rstd;
        if (stats && chunk == 0) {
            stats[((size_t)n * G + tid) * 2] = mean;
            stats[((size_t)n * G + tid) * 2 + 1] = rstd;
        }
    }
    __syncthreads();
    float mu[4], rs[4], ga[4], be[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = col * 4 + e;
        mu[e] = ms[0][c / cpg];
        rs[e] = ms[1][c / cpg];
        ga[e] = gamma[c];
        be[e] = beta[c];
    }
    bf16_t* ob = out + (size_t)n * HW * C;
    const int p0 = chunk * GN_PX, p1 = p0 + GN_PX < HW ? p0 + GN_PX : HW;
    for (int px = p0 + pl; px < p1; px += lanes) {
        const float4 v = *(const float4*)(xb + (size_t)px * C + col * 4);
        const float ve[4] = {v.x, v.y, v.z, v.w};
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = (ve[e] - mu[e]) * rs[e] * ga[e] + be[e];
            if (silu) y[e] = y[e] / (1.f + __expf(-y[e]));
        }
        *(uint2*)(ob + (size_t)px * C + col * 4) = uint2{pack16s(y[0], y[1]), pack16s(y[2], y[3])};
    }
}

// ---- row softmax --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vae_softmax_kernel(const float* __restrict__ sc, int lds, bf16_t* __restrict__ pr, int ldp, int T) {
    __shared__ float red[4];
    __shared__ float bc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = sc + (size_t)blockIdx.x * lds;
    bf16_t* orow = pr + (size_t)blockIdx.x * ldp;
    float mx = -INFINITY;
    for (int i = tid; i < T; i += 256) mx = fmaxf(mx, row[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (tid == 0) bc = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    mx = bc;
    float s = 0.f;
    for (int i = tid; i < T; i += 256) s += __expf(row[i] - mx);
    s = wave_sum(s);
    __syncthreads();                      // red is free again: thread 0 has read it
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float inv = 1.f / (((red[0] + red[1]) + red[2]) + red[3]);
    for (int i = tid; i < T; i += 256) orow[i] = cvt16(__expf(row[i] - mx) * inv);
}

#if MAPDIT_DT == 0
// ---- the encoder's pointwise kernels: fp32 and bytes only, so they are built once (no _f16 twin) -------------------------------------
// uint8 [N, H, W, C] -> fp32 NHWC, ToTensor + Normalize(0.5, 0.5): ((float)u / 255 - 0.5) / 0.5 in that order, IEEE division (the
// one-multiply form u * (2 / 255) - 1 rounds differently on 111 of the 256 bytes).  flip[n] != 0 mirrors sample n left-right.
__global__ __launch_bounds__(256) void vae_prepare_u8_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ flip,
                                                            float* __restrict__ out, long total, int H, int W, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long pix = idx / C;
    const int x = (int)(pix % W);
    const long row = pix / W;                              // n * H + y
    const int n = (int)(row / H);
    const int xs = flip && flip[n] ? W - 1 - x : x;
    const float u = (float)img[(row * W + xs) * C + c];
    out[idx] = (u / 255.f - 0.5f) / 0.5f;
}

// DiagonalGaussianDistribution: moments fp32 NHWC [N, hw, 2L] -> mean, std (, logvar) fp32 NCHW [N, L, hw]; one thread per output element.
// The clamp is written with comparisons so that a NaN log-variance stays NaN (fminf / fmaxf would drop it).
__global__ __launch_bounds__(256) void vae_posterior_kernel(const float* __restrict__ mom, float* __restrict__ mean, float* __restrict__ std,
                                                           float* __restrict__ logvar, long total, int hw, int L) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int px = (int)(idx % hw);
    const long nl = idx / hw;
    const int l = (int)(nl % L);
    const long n = nl / L;
    const float* mp = mom + (n * hw + px) * 2 * L;
    const float raw = mp[L + l];
    const float lv = raw < -30.f ? -30.f : raw > 20.f ? 20.f : raw;
    mean[idx] = mp[l];
    std[idx] = expf(0.5f * lv);
    if (logvar) logvar[idx] = lv;
}

// Per-channel fp64 sums of m, m * m and s * s, added to acc[l][0..2]: one workgroup per channel walks the batch [N, L, hw] sample by
// sample.  A sample's sums are formed in a fixed order - thread (element stride 256), wave (xor shuffles), the four waves through LDS -
// and added to the running sums by thread 0, in sample order: no atomics, and the result is a function of the sequence of samples,
// not of how it is cut into batches.
__global__ __launch_bounds__(256) void vae_stats_accumulate_kernel(const float* __restrict__ mean, const float* __restrict__ std, int N, int L,
                                                                  int hw, double* __restrict__ acc) {
    __shared__ double red[3][4];
    const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double run[3] = {0.0, 0.0, 0.0};
    if (tid == 0)
        for (int j = 0; j < 3; ++j) run[j] = acc[l * 3 + j];
    for (int n = 0; n < N; ++n) {
        const size_t base = ((size_t)n * L + l) * hw;
        double a = 0.0, b = 0.0, c = 0.0;
        for (int i = tid; i < hw; i += 256) {
            const double m = (double)mean[base + i], s = (double)std[base + i];
            a += m;
            b += m * m;
            c += s * s;
        }
        a = wave_sum_d(a);
        b = wave_sum_d(b);
        c = wave_sum_d(c);
        if (lane == 0) {
            red[0][wave] = a;
            red[1][wave] = b;
            red[2][wave] = c;
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < 3; ++j) run[j] += ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
        __syncthreads();                                   // red is free for the next sample
    }
    if (tid == 0)
        for (int j = 0; j < 3; ++j) acc[l * 3 + j] = run[j];
}

// mean_c = sum m / n, std_c = sqrt(sum s^2 / n + sum m^2 / n - mean_c^2) in fp64 (the reference's E[s^2] + E[(m - mean_c)^2]), stored as fp32
__global__ void vae_stats_finish_kernel(const double* __restrict__ acc, double count, float* __restrict__ ch_mean, float* __restrict__ ch_std, int L) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const double m = acc[l * 3] / count;
    double var = acc[l * 3 + 2] / count + (acc[l * 3 + 1] / count - m * m);
    var = var < 0.0 ? 0.0 : var;                           // (a NaN stays a NaN)
    ch_mean[l] = (float)m;
    ch_std[l] = (float)sqrt(var);
}
#endif

MD_NS_CLOSE

// ---- entry points -----------------------------------------------------------------------------------------------------------------
// mapdit_vae_conv (Hin = Win = 0) and mapdit_vae_conv_down (the input size) are one launch path: only the coordinate map differs.
static int vae_conv_launch(const char* who, const mapdit_vae_conv_t* a, int Hin, int Win, bool down, void* stream) {
    MD_CHECK(a && a->in && a->w && a->bias && a->out, "%s: null argument", who);
    if (down) MD_CHECK(a->k == 3, "%s: k=%d (the downsample is a 3 x 3 convolution)", who, a->k);
    else MD_CHECK(a->k == 1 || a->k == 3, "%s: k=%d (1 or 3)", who, a->k);
    MD_CHECK(a->N > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cout > 0, "%s: empty shape N=%d H=%d W=%d Cin=%d Cout=%d", who, a->N, a->H,
             a->W, a->Cin, a->Cout);
    MD_CHECK(a->in_kind >= MAPDIT_VAE_IN_16 && a->in_kind <= MAPDIT_VAE_IN_F32_NCHW, "%s: bad in_kind %d", who, a->in_kind);
    MD_CHECK(a->out_kind >= MAPDIT_VAE_OUT_F32 && a->out_kind <= MAPDIT_VAE_OUT_16, "%s: bad out_kind %d", who, a->out_kind);
    if (down) {
        MD_CHECK(!a->up2, "%s: up2=%d (a downsample reads no upsampled input)", who, a->up2);
        MD_CHECK(Hin >= 2 && Win >= 2, "%s: input of %d x %d (2 x 2 at the least)", who, Hin, Win);
        MD_CHECK(a->H == Hin / 2 && a->W == Win / 2, "%s: output %d x %d of a %d x %d input (%d x %d expected: half, rounded down)", who, a->H,
                 a->W, Hin, Win, Hin / 2, Win / 2);
        MD_CHECK((long)a->N * Hin * Win < (1L << 31), "%s: %ld input pixels are too many", who, (long)a->N * Hin * Win);
    } else {
        MD_CHECK(!a->up2 || (a->H % 2 == 0 && a->W % 2 == 0), "%s: up2 needs even H=%d, W=%d", who, a->H, a->W);
    }
    MD_CHECK(!(a->res && a->out_kind == MAPDIT_VAE_OUT_F32_NCHW), "%s: no residual with the NCHW store", who);
    const long M = (long)a->N * a->H * a->W;
    MD_CHECK(M * a->Cout < (1L << 40) && M < (1L << 31), "%s: %ld output pixels are too many", who, M);
    const int up2 = a->up2 ? 1 : 0, st = down ? 2 : 1, pad = down ? 0 : a->k >> 1;
    const md_conv_t p{a->in, (const bf16_t*)a->w, a->bias, a->res, a->out, a->in_kind, a->out_kind,
                      down ? Hin : a->H >> up2, down ? Win : a->W >> up2, down ? Hin : a->H, down ? Win : a->W, up2,
                      a->k, a->k, st, pad, pad, a->H, a->W, a->Cin, a->Cout, (int)((long)a->k * a->k * a->Cin), M, a->Cout, 0, 0};
    // the MFMA path exactly for 64-channel multiples on both sides, NHWC, aligned; the wide tile exactly when Cout % 128 == 0
    const bool aligned = !(((uintptr_t)a->in | (uintptr_t)a->w) & 15);
    const bool mfma = a->Cin % 64 == 0 && a->Cout % 64 == 0 && a->in_kind != MAPDIT_VAE_IN_F32_NCHW && a->out_kind != MAPDIT_VAE_OUT_F32_NCHW && aligned;
    return MD_SYM(conv_launch)(who, &p, !mfma ? MD_CONV_PLAIN : a->Cout % 128 == 0 ? MD_CONV_128 : MD_CONV_64, stream);
}

extern "C" int MD_SYM(vae_conv)(const mapdit_vae_conv_t* a, void* stream) { return vae_conv_launch("vae_conv", a, 0, 0, false, stream); }

extern "C" int MD_SYM(vae_conv_down)(const mapdit_vae_conv_t* a, int Hin, int Win, void* stream) {
    return vae_conv_launch("vae_conv_down", a, Hin, Win, true, stream);
}

extern "C" int MD_SYM(vae_groupnorm)(const float* x, const float* gamma, const float* beta, float eps, int silu, uint16_t* out, float* stats,
                                     int N, int HW, int C, int G, void* scratch, size_t scratch_bytes, void* stream) {
    MD_CHECK(x && gamma && beta && out, "vae_groupnorm: null argument");
    MD_CHECK(N > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0, "vae_groupnorm: N=%d HW=%d C=%d must be positive and C a multiple of G=%d", N, HW, C, G);
    MD_CHECK((long)N * G < (1L << 31) && N < 65536, "vae_groupnorm: too many samples / groups");
    hipStream_t st = (hipStream_t)stream;
    const int nchunks = cdiv(HW, GN_PX);
    const bool split = scratch && scratch_bytes >= (size_t)N * nchunks * G * 2 * sizeof(double) && !((uintptr_t)scratch & 7) && C % 4 == 0 &&
                       C / 4 <= 256 && 256 % (C / 4) == 0 && G <= 256 && !((uintptr_t)x & 15) && !((uintptr_t)out & 7);
    if (split) {
        const dim3 grid((unsigned)nchunks, (unsigned)N);
        vae_gn_stats_kernel<<<grid, 256, 0, st>>>(x, (double*)scratch, HW, C, G);
        vae_gn_apply_kernel<<<grid, 256, 0, st>>>(x, (const double*)scratch, gamma, beta, eps, silu, (bf16_t*)out, stats, HW, C, G);
    } else {
        vae_groupnorm_kernel<<<N * G, 256, 0, st>>>(x, gamma, beta, eps, silu, (bf16_t*)out, stats, HW, C, G);
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int MD_SYM(vae_softmax)(const float* scores, int lds, uint16_t* probs, int ldp, int rows, int T, void* stream) {
    MD_CHECK(scores && probs && rows > 0 && T > 0 && lds >= T && ldp >= T, "vae_softmax: null / empty argument (rows=%d T=%d lds=%d ldp=%d)", rows, T,
             lds, ldp);
    vae_softmax_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(scores, lds, (bf16_t*)probs, ldp, T);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

// ---- the pointwise entry points of the encoder (one build) --------------------------------------------------------------------------
#if MAPDIT_DT == 0
extern "C" int mapdit_vae_prepare_u8(const uint8_t* img, const uint8_t* flip, float* out, int N, int H, int W, int C, void* stream) {
    MD_CHECK(img && out, "vae_prepare_u8: null argument");
    MD_CHECK(N > 0 && H > 0 && W > 0 && C > 0, "vae_prepare_u8: N=%d, H=%d, W=%d, C=%d must be positive", N, H, W, C);
    const long total = (long)N * H * W * C;
    MD_CHECK(total < (1L << 38), "vae_prepare_u8: %ld elements are too many for one call", total);
    vae_prepare_u8_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(img, flip, out, total, H, W, C);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_vae_posterior(const float* moments, float* mean, float* std, float* logvar, int N, int hw, int L, void* stream) {
    MD_CHECK(moments && mean && std, "vae_posterior: null argument");
    MD_CHECK(N > 0 && hw > 0 && L > 0, "vae_posterior: N=%d, hw=%d, L=%d must be positive", N, hw, L);
    const long total = (long)N * hw * L;
    MD_CHECK(total < (1L << 38), "vae_posterior: %ld elements are too many for one call", total);
    vae_posterior_kernel<<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(moments, mean, std, logvar, total, hw, L);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_vae_stats_accumulate(const float* mean, const float* std, int N, int L, int hw, double* acc, void* stream) {
    MD_CHECK(mean && std && acc, "vae_stats_accumulate: null argument");
    MD_CHECK(N > 0 && L > 0 && hw > 0, "vae_stats_accumulate: N=%d, L=%d, hw=%d must be positive", N, L, hw);
    MD_CHECK(!((uintptr_t)acc & 7), "vae_stats_accumulate: acc must be 8-byte aligned");
    vae_stats_accumulate_kernel<<<L, 256, 0, (hipStream_t)stream>>>(mean, std, N, L, hw, acc);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" int mapdit_vae_stats_finish(const double* acc, double count, float* ch_mean, float* ch_std, int L, void* stream) {
    MD_CHECK(acc && ch_mean && ch_std, "vae_stats_finish: null argument");
    MD_CHECK(L > 0 && count > 0.0, "vae_stats_finish: L=%d and count=%g must be positive", L, count);
    vae_stats_finish_kernel<<<cdiv(L, 64), 64, 0, (hipStream_t)stream>>>(acc, count, ch_mean, ch_std, L);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
#endif

// ---- the two plans ------------------------------------------------------------------------------------------------------------------
namespace {
struct VaePlan {
    int C[4];          // widths in execution order: the decoder walks block_out_channels reversed, the encoder as listed
    int nb;
    size_t maxE;       // largest activation, elements
    size_t off_x, off_y, off_h, off_a, off_qkv, off_s, off_p, off_gn, gn_bytes, total;
};

// the config checks both directions share; fills nb and C.  0 = ok; otherwise the message is set
int vae_plan_config(const mapdit_vae_config_t* cfg, int N, int h, int w, bool reversed, VaePlan* pl) {
    MD_CHECK(cfg, "vae: null config");
    MD_CHECK(N > 0 && h > 0 && w > 0, "vae: N=%d, h=%d, w=%d must be positive", N, h, w);
    MD_CHECK(cfg->num_blocks >= 1 && cfg->num_blocks <= 4, "vae: num_blocks=%d (1..4 block widths)", cfg->num_blocks);
    MD_CHECK(cfg->latent_channels > 0 && cfg->out_channels > 0 && cfg->layers_per_block >= 1 && cfg->layers_per_block <= 16,
             "vae: latent_channels=%d, out_channels=%d, layers_per_block=%d", cfg->latent_channels, cfg->out_channels, cfg->layers_per_block);
    MD_CHECK(cfg->norm_num_groups > 0, "vae: norm_num_groups=%d must be positive", cfg->norm_num_groups);
    const int ch[4] = {cfg->ch0, cfg->ch1, cfg->ch2, cfg->ch3};
    pl->nb = cfg->num_blocks;
    for (int i = 0; i < pl->nb; ++i) {
        const int c = ch[reversed ? pl->nb - 1 - i : i];
        MD_CHECK(c > 0 && c % cfg->norm_num_groups == 0, "vae: channel width %d is not a multiple of the norm groups (%d)", c, cfg->norm_num_groups);
        MD_CHECK(c % 8 == 0, "vae: channel width %d is not a multiple of 8 (16-bit operand rows of 16 bytes)", c);
        pl->C[i] = c;
    }
    return MAPDIT_OK;
}

// the workspace of either direction: three fp32 and one 16-bit activation of maxE elements, the attention buffers for T tokens of
// width Cmid, and the split GroupNorm's partial sums for images of max_hw pixels
void vae_plan_layout(VaePlan* pl, size_t maxE, int N, size_t T, int Cmid, size_t max_hw, int G) {
    pl->maxE = maxE;
    size_t o = 0;
    pl->off_x = o; o += md_up256(maxE * 4);
    pl->off_y = o; o += md_up256(maxE * 4);
    pl->off_h = o; o += md_up256(maxE * 4);
    pl->off_a = o; o += md_up256(maxE * 2);
    pl->off_qkv = o; o += md_up256((size_t)N * T * 3 * Cmid * 2);
    pl->off_s = o; o += md_up256(T * T * 4);
    pl->off_p = o; o += md_up256(T * T * 2);
    // partial sums of the split GroupNorm: per sample, 1,024-pixel chunk of the largest image and group, two fp64
    pl->gn_bytes = (size_t)N * (size_t)cdiv((long)max_hw, GN_PX) * G * 2 * sizeof(double);
    pl->off_gn = o; o += md_up256(pl->gn_bytes);
    pl->total = o;
}

int vae_plan(const mapdit_vae_config_t* cfg, int N, int h, int w, VaePlan* pl) {
    MD_TRY(vae_plan_config(cfg, N, h, w, true, pl));
    MD_CHECK((long)h * w % 8 == 0, "vae: h*w = %ld tokens in the mid-block attention must be a multiple of 8 (operand alignment of its GEMMs)", (long)h * w);
    MD_CHECK((long)N * h * w * (1L << (2 * (pl->nb - 1))) < (1L << 31), "vae: N=%d latents of %d x %d are too many output pixels for one call", N, h, w);
    size_t px = (size_t)N * h * w, maxE = px * (size_t)pl->C[0];
    int cin = pl->C[0];
    for (int i = 0; i < pl->nb; ++i) {
        const size_t e = px * (size_t)(cin > pl->C[i] ? cin : pl->C[i]);
        maxE = e > maxE ? e : maxE;
        cin = pl->C[i];
        if (i < pl->nb - 1) {
            px *= 4;
            maxE = px * (size_t)cin > maxE ? px * (size_t)cin : maxE;
        }
    }
    vae_plan_layout(pl, maxE, N, (size_t)h * w, pl->C[0], px / N, cfg->norm_num_groups);
    return MAPDIT_OK;
}

// the encoder: N images of H x W
int vae_encode_plan(const mapdit_vae_config_t* cfg, int N, int H, int W, VaePlan* pl) {
    MD_TRY(vae_plan_config(cfg, N, H, W, false, pl));
    const int s = 1 << (pl->nb - 1);
    MD_CHECK(H % s == 0 && W % s == 0, "vae encode: an image of %d x %d is not a multiple of %d (2^(num_blocks - 1): every downsample halves an even size)", H, W, s);
    const long T = (long)(H / s) * (W / s);
    MD_CHECK(T % 8 == 0, "vae encode: (H / %d) * (W / %d) = %ld tokens in the mid-block attention must be a multiple of 8 (operand alignment of its GEMMs)", s, s, T);
    MD_CHECK((long)N * H * W < (1L << 31), "vae encode: N=%d images of %d x %d are too many pixels for one call", N, H, W);
    size_t px = (size_t)N * H * W, maxE = px * (size_t)pl->C[0];
    int cin = pl->C[0];
    for (int i = 0; i < pl->nb; ++i) {
        const size_t e = px * (size_t)(cin > pl->C[i] ? cin : pl->C[i]);
        maxE = e > maxE ? e : maxE;
        cin = pl->C[i];
        if (i < pl->nb - 1) px /= 4;
    }
    const size_t mom = px * 2 * (size_t)cfg->latent_channels;          // conv_out / quant_conv outputs
    maxE = mom > maxE ? mom : maxE;
    vae_plan_layout(pl, maxE, N, (size_t)T, pl->C[pl->nb - 1], (size_t)H * W, cfg->norm_num_groups);
    return MAPDIT_OK;
}

// What a plan runs with: the workspace's buffers and the launches both directions are made of.  The resnet and the mid-block
// attention are the same code in the decoder and the encoder; X holds the residual stream on entry and on return.
struct VaeRun {
    const char* who;
    int N, G;
    float eps;
    void* stream;
    float *X, *Y, *Hb;
    uint16_t *A16, *QKV;
    float* S;
    uint16_t* P;
    void* gn_scratch;
    size_t gn_bytes;

    VaeRun(const char* who_, const mapdit_vae_config_t* cfg, const VaePlan& pl, int N_, void* workspace, void* stream_)
        : who(who_), N(N_), G(cfg->norm_num_groups), eps(cfg->norm_eps), stream(stream_) {
        char* ws = (char*)workspace;
        X = (float*)(ws + pl.off_x);
        Y = (float*)(ws + pl.off_y);
        Hb = (float*)(ws + pl.off_h);
        A16 = (uint16_t*)(ws + pl.off_a);
        QKV = (uint16_t*)(ws + pl.off_qkv);
        S = (float*)(ws + pl.off_s);
        P = (uint16_t*)(ws + pl.off_p);
        gn_scratch = ws + pl.off_gn;
        gn_bytes = pl.gn_bytes;
    }
    void swap_xy() {
        float* t = X;
        X = Y;
        Y = t;
    }
    int conv(const void* in, int in_kind, const void* wgt, const void* bias, const float* res, void* o, int out_kind, int H, int W, int Cin, int Cout,
             int k, int up2) const {
        const mapdit_vae_conv_t a{in, in_kind, (const uint16_t*)wgt, (const float*)bias, res, o, out_kind, N, H, W, Cin, Cout, k, up2};
        return MD_SYM(vae_conv)(&a, stream);
    }
    // [N, Hin, Win, C] -> [N, Hin / 2, Win / 2, C]
    int conv_down(const void* in, int in_kind, const void* wgt, const void* bias, void* o, int out_kind, int Hin, int Win, int Cin, int Cout) const {
        const mapdit_vae_conv_t a{in, in_kind, (const uint16_t*)wgt, (const float*)bias, nullptr, o, out_kind, N, Hin / 2, Win / 2, Cin, Cout, 3, 0};
        return MD_SYM(vae_conv_down)(&a, Hin, Win, stream);
    }
    int gn(const float* x, const void* g, const void* b, int silu, int HW, int C) const {
        return MD_SYM(vae_groupnorm)(x, (const float*)g, (const float*)b, eps, silu, A16, nullptr, N, HW, C, G, gn_scratch, gn_bytes, stream);
    }
    // X [N, H, W, cin] -> X [N, H, W, cout]; r: the resnet's MAPDIT_VAE_NUM_RESNET slots, rix its number in execution order
    int resnet(const void* const* r, int rix, int H, int W, int cin, int cout) const {
        const bool sc = cin != cout;
        MD_CHECK(!sc || (r[MAPDIT_VAE_R_SC_W] && r[MAPDIT_VAE_R_SC_B]), "%s: resnet %d maps %d -> %d channels and has no conv_shortcut", who, rix, cin, cout);
        MD_TRY(gn(X, r[MAPDIT_VAE_R_N1_G], r[MAPDIT_VAE_R_N1_B], 1, H * W, cin));
        MD_TRY(conv(A16, MAPDIT_VAE_IN_16, r[MAPDIT_VAE_R_C1_W], r[MAPDIT_VAE_R_C1_B], nullptr, Hb, MAPDIT_VAE_OUT_F32, H, W, cin, cout, 3, 0));
        MD_TRY(gn(Hb, r[MAPDIT_VAE_R_N2_G], r[MAPDIT_VAE_R_N2_B], 1, H * W, cout));
        if (sc) MD_TRY(conv(X, MAPDIT_VAE_IN_F32, r[MAPDIT_VAE_R_SC_W], r[MAPDIT_VAE_R_SC_B], nullptr, Y, MAPDIT_VAE_OUT_F32, H, W, cin, cout, 1, 0));
        // (same widths: the residual is read and the sum written in place, element by element, by the thread that owns it)
        MD_TRY(conv(A16, MAPDIT_VAE_IN_16, r[MAPDIT_VAE_R_C2_W], r[MAPDIT_VAE_R_C2_B], sc ? Y : X, X, MAPDIT_VAE_OUT_F32, H, W, cout, cout, 3, 0));
        return MAPDIT_OK;
    }
    // the mid block's single-head attention over the T = H * W pixels of each sample, X += out(softmax(q k^T / sqrt(C)) v)
    int attention(const void* gn_g, const void* gn_b, const void* qkv_w, const void* qkv_b, const void* out_w, const void* out_b, int H, int W,
                  int C0) const {
        const int T = H * W;
        MD_TRY(gn(X, gn_g, gn_b, 0, T, C0));
        MD_TRY(conv(A16, MAPDIT_VAE_IN_16, qkv_w, qkv_b, nullptr, QKV, MAPDIT_VAE_OUT_16, H, W, C0, 3 * C0, 1, 0));
        for (int n = 0; n < N; ++n) {
            const uint16_t* qn = QKV + (size_t)n * T * 3 * C0;
            mapdit_epilogue_t e{};
            e.kind = MAPDIT_EPI_STORE_F32;
            e.out = S;
            e.ldo = T;
            e.alpha = 1.f / sqrtf((float)C0);
            MD_TRY(MD_SYM_GEMM(MAPDIT_NT, T, T, C0, qn, 3 * C0, qn + C0, 3 * C0, &e, stream));
            MD_TRY(MD_SYM(vae_softmax)(S, T, P, T, T, T, stream));
            mapdit_epilogue_t e2{};
            e2.kind = MAPDIT_EPI_STORE_F32;
            e2.out = Hb + (size_t)n * T * C0;
            e2.ldo = C0;
            e2.alpha = 1.f;
            MD_TRY(MD_SYM_GEMM(MAPDIT_NN, T, C0, T, P, T, qn + 2 * C0, 3 * C0, &e2, stream));
        }
        return conv(Hb, MAPDIT_VAE_IN_F32, out_w, out_b, X, X, MAPDIT_VAE_OUT_F32, H, W, C0, C0, 1, 0);
    }
};

// every slot but a resnet's conv_shortcut pair must be set
int vae_check_table(const char* who, const void* const* wt, int nglobal, int nres, int ntail) {
    const int nslots = nglobal + nres * MAPDIT_VAE_NUM_RESNET + ntail;
    for (int i = 0; i < nslots; ++i) {
        const int rs = i - nglobal;
        const bool optional = rs >= 0 && rs < nres * MAPDIT_VAE_NUM_RESNET &&
                              (rs % MAPDIT_VAE_NUM_RESNET == MAPDIT_VAE_R_SC_W || rs % MAPDIT_VAE_NUM_RESNET == MAPDIT_VAE_R_SC_B);
        MD_CHECK(wt[i] || optional, "%s: weight slot %d is null", who, i);
    }
    return MAPDIT_OK;
}
}  // namespace

#if MAPDIT_DT == 0
extern "C" size_t mapdit_vae_workspace_bytes(const mapdit_vae_config_t* cfg, int N, int h, int w) {
    VaePlan pl;
    return vae_plan(cfg, N, h, w, &pl) == MAPDIT_OK ? pl.total : 0;
}

extern "C" size_t mapdit_vae_encode_workspace_bytes(const mapdit_vae_config_t* cfg, int N, int H, int W) {
    VaePlan pl;
    return vae_encode_plan(cfg, N, H, W, &pl) == MAPDIT_OK ? pl.total : 0;
}
#endif

extern "C" int MD_SYM(vae_decode)(const mapdit_vae_config_t* cfg, const void* const* wt, const float* z, float* out, int N, int h, int w,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    VaePlan pl;
    MD_TRY(vae_plan(cfg, N, h, w, &pl));
    MD_CHECK(wt && z && out && workspace, "vae_decode: null argument");
    MD_CHECK(workspace_bytes >= pl.total, "vae_decode: workspace of %zu bytes, %zu needed (mapdit_vae_workspace_bytes)", workspace_bytes, pl.total);
    MD_CHECK(!((uintptr_t)workspace & 255), "vae_decode: the workspace must be 256-byte aligned");
    const int nres = 2 + pl.nb * (cfg->layers_per_block + 1);
    MD_TRY(vae_check_table("vae_decode", wt, MAPDIT_VAE_NUM_GLOBAL, nres, (pl.nb - 1) * MAPDIT_VAE_NUM_UP));
    VaeRun r("vae_decode", cfg, pl, N, workspace, stream);
    int rix = 0;      // resnets in execution order
    auto resnet = [&](int H, int W, int cin, int cout) {
        const int i = rix++;
        return r.resnet(wt + MAPDIT_VAE_NUM_GLOBAL + i * MAPDIT_VAE_NUM_RESNET, i, H, W, cin, cout);
    };

    int H = h, W = w;
    const int C0 = pl.C[0], L = cfg->latent_channels;
    // post_quant_conv (reads z as NCHW) and conv_in
    MD_TRY(r.conv(z, MAPDIT_VAE_IN_F32_NCHW, wt[MAPDIT_VAE_W_PQ_W], wt[MAPDIT_VAE_W_PQ_B], nullptr, r.Hb, MAPDIT_VAE_OUT_F32, H, W, L, L, 1, 0));
    MD_TRY(r.conv(r.Hb, MAPDIT_VAE_IN_F32, wt[MAPDIT_VAE_W_CONV_IN_W], wt[MAPDIT_VAE_W_CONV_IN_B], nullptr, r.X, MAPDIT_VAE_OUT_F32, H, W, L, C0, 3, 0));
    // mid block
    MD_TRY(resnet(H, W, C0, C0));
    MD_TRY(r.attention(wt[MAPDIT_VAE_W_ATTN_GN_G], wt[MAPDIT_VAE_W_ATTN_GN_B], wt[MAPDIT_VAE_W_ATTN_QKV_W], wt[MAPDIT_VAE_W_ATTN_QKV_B],
                        wt[MAPDIT_VAE_W_ATTN_OUT_W], wt[MAPDIT_VAE_W_ATTN_OUT_B], H, W, C0));
    MD_TRY(resnet(H, W, C0, C0));
    // up blocks
    int cin = C0;
    const void* const* ups = wt + MAPDIT_VAE_NUM_GLOBAL + nres * MAPDIT_VAE_NUM_RESNET;
    for (int i = 0; i < pl.nb; ++i) {
        const int cout = pl.C[i];
        for (int j = 0; j <= cfg->layers_per_block; ++j) {
            MD_TRY(resnet(H, W, cin, cout));
            cin = cout;
        }
        if (i < pl.nb - 1) {
            const void* const* u = ups + i * MAPDIT_VAE_NUM_UP;
            H *= 2;
            W *= 2;
            MD_TRY(r.conv(r.X, MAPDIT_VAE_IN_F32, u[MAPDIT_VAE_U_W], u[MAPDIT_VAE_U_B], nullptr, r.Y, MAPDIT_VAE_OUT_F32, H, W, cout, cout, 3, 1));
            r.swap_xy();
        }
    }
    MD_TRY(r.gn(r.X, wt[MAPDIT_VAE_W_NORM_OUT_G], wt[MAPDIT_VAE_W_NORM_OUT_B], 1, H * W, cin));
    MD_TRY(r.conv(r.A16, MAPDIT_VAE_IN_16, wt[MAPDIT_VAE_W_CONV_OUT_W], wt[MAPDIT_VAE_W_CONV_OUT_B], nullptr, out, MAPDIT_VAE_OUT_F32_NCHW, H, W, cin,
                   cfg->out_channels, 3, 0));
    return MAPDIT_OK;
}

// x [N, H, W, C] (MAPDIT_VAE_IN_F32) or [N, C, H, W] (MAPDIT_VAE_IN_F32_NCHW) -> mean, std fp32 [N, L, H / s, W / s]
extern "C" int MD_SYM(vae_encode)(const mapdit_vae_config_t* cfg, const void* const* wt, const float* x, int x_kind, float* mean, float* std, int N,
                                  int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    VaePlan pl;
    MD_TRY(vae_encode_plan(cfg, N, H, W, &pl));
    MD_CHECK(wt && x && mean && std && workspace, "vae_encode: null argument");
    MD_CHECK(x_kind == MAPDIT_VAE_IN_F32 || x_kind == MAPDIT_VAE_IN_F32_NCHW, "vae_encode: x_kind=%d (MAPDIT_VAE_IN_F32 or MAPDIT_VAE_IN_F32_NCHW)", x_kind);
    MD_CHECK(workspace_bytes >= pl.total, "vae_encode: workspace of %zu bytes, %zu needed (mapdit_vae_encode_workspace_bytes)", workspace_bytes, pl.total);
    MD_CHECK(!((uintptr_t)workspace & 255), "vae_encode: the workspace must be 256-byte aligned");
    const int nres = pl.nb * cfg->layers_per_block + 2;
    MD_TRY(vae_check_table("vae_encode", wt, MAPDIT_VAE_E_NUM_GLOBAL, nres, (pl.nb - 1) * MAPDIT_VAE_NUM_DOWN));
    VaeRun r("vae_encode", cfg, pl, N, workspace, stream);
    int rix = 0;
    auto resnet = [&](int h, int w, int cin, int cout) {
        const int i = rix++;
        return r.resnet(wt + MAPDIT_VAE_E_NUM_GLOBAL + i * MAPDIT_VAE_NUM_RESNET, i, h, w, cin, cout);
    };

    const int L2 = 2 * cfg->latent_channels;
    MD_TRY(r.conv(x, x_kind, wt[MAPDIT_VAE_E_CONV_IN_W], wt[MAPDIT_VAE_E_CONV_IN_B], nullptr, r.X, MAPDIT_VAE_OUT_F32, H, W, cfg->out_channels, pl.C[0], 3, 0));
    // down blocks
    int cin = pl.C[0];
    const void* const* downs = wt + MAPDIT_VAE_E_NUM_GLOBAL + nres * MAPDIT_VAE_NUM_RESNET;
    for (int i = 0; i < pl.nb; ++i) {
        const int cout = pl.C[i];
        for (int j = 0; j < cfg->layers_per_block; ++j) {
            MD_TRY(resnet(H, W, cin, cout));
            cin = cout;
        }
        if (i < pl.nb - 1) {
            const void* const* d = downs + i * MAPDIT_VAE_NUM_DOWN;
            MD_TRY(r.conv_down(r.X, MAPDIT_VAE_IN_F32, d[MAPDIT_VAE_D_W], d[MAPDIT_VAE_D_B], r.Y, MAPDIT_VAE_OUT_F32, H, W, cout, cout));
            r.swap_xy();
            H /= 2;
            W /= 2;
        }
    }
    // mid block
    MD_TRY(resnet(H, W, cin, cin));
    MD_TRY(r.attention(wt[MAPDIT_VAE_E_ATTN_GN_G], wt[MAPDIT_VAE_E_ATTN_GN_B], wt[MAPDIT_VAE_E_ATTN_QKV_W], wt[MAPDIT_VAE_E_ATTN_QKV_B],
                        wt[MAPDIT_VAE_E_ATTN_OUT_W], wt[MAPDIT_VAE_E_ATTN_OUT_B], H, W, cin));
    MD_TRY(resnet(H, W, cin, cin));
    // conv_norm_out + SiLU, conv_out, quant_conv, the posterior head
    MD_TRY(r.gn(r.X, wt[MAPDIT_VAE_E_NORM_OUT_G], wt[MAPDIT_VAE_E_NORM_OUT_B], 1, H * W, cin));
    MD_TRY(r.conv(r.A16, MAPDIT_VAE_IN_16, wt[MAPDIT_VAE_E_CONV_OUT_W], wt[MAPDIT_VAE_E_CONV_OUT_B], nullptr, r.Hb, MAPDIT_VAE_OUT_F32, H, W, cin, L2, 3, 0));
    MD_TRY(r.conv(r.Hb, MAPDIT_VAE_IN_F32, wt[MAPDIT_VAE_E_QUANT_W], wt[MAPDIT_VAE_E_QUANT_B], nullptr, r.Y, MAPDIT_VAE_OUT_F32, H, W, L2, L2, 1, 0));
    return mapdit_vae_posterior(r.Y, mean, std, nullptr, N, H * W, cfg->latent_channels, stream);
}
