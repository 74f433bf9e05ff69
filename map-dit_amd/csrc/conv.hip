// The library's one convolution: an implicit GEMM on the MFMA in two tile forms, a plain kernel for every other shape, and the host
// launcher the entry points call (common.h, md_conv_t / conv_launch; mapdit_vae_conv, mapdit_vae_conv_down and mapdit_inc_conv fill the
// block and choose the tile - DESIGN.md §4).  Built once per 16-bit operand format (csrc/Makefile).
//
// out[m][co] = sum_K A[m][K] * w[co][K] with m = (n, y, x) of the OUTPUT flattened and K = (ky, kx, c) flattened to Ktot = kh * kw * Cin:
// the weight is a plain row-major [Cout][Ktot] B operand, the A operand is gathered.
// Coordinate map.  Output pixel (y, x), tap (ky, kx) reads logical input (y * st + ky - ph, x * st + kx - pw), tested against the
// logical extent (Hb, Wb) and stored at (yy >> up2, xx >> up2) of a [N, Hs, Ws, Cin] source.  An out-of-image tap, a row past M, a
// granule past Ktot and a weight row past Cout stage zeros without forming an address.  A tile of 128 consecutive m straddles image
// rows and, for small images, samples: each staged row derives (n, y, x) from its own m - never from the flat index.
// K is staged in GRANULES of 16 channels (Cin % 16 == 0): a granule lies inside one tap (one bounds decision, two 16-byte loads), a
// 64-wide K tile is four granules that may belong to different taps (with Cin % 64 == 0 they are 64 channels of ONE tap), and the
// granules of the last tile past Ktot are zeros on both operands.  Global -> registers -> LDS -> v_mfma_f32_16x16x32; LDS rows are
// padded to 72 elements (144 B: 16-byte aligned, consecutive rows 4 banks apart).
// The K order of an output element is the tile order and the MFMA's own: it does not depend on the tile form, on where the pixel falls
// in a tile or on N, so a sample alone and in a batch gives the same bits.
#include "common.h"

MD_NS_OPEN

constexpr int CBM = 128, CBK = 64, CLD = CBK + 8;

// 16 consecutive channels of one input pixel as 16-bit operands (8 packed words)
template <int IN_F32> __device__ __forceinline__ void load16(const void* in, size_t elem, uint4& lo, uint4& hi) {
    if constexpr (IN_F32) {
        const float4* p = (const float4*)((const float*)in + elem);
        const float4 a = p[0], b = p[1], c = p[2], d = p[3];
        lo = uint4{pack16s(a.x, a.y), pack16s(a.z, a.w), pack16s(b.x, b.y), pack16s(b.z, b.w)};
        hi = uint4{pack16s(c.x, c.y), pack16s(c.z, c.w), pack16s(d.x, d.y), pack16s(d.z, d.w)};
    } else {
        const uint4* p = (const uint4*)((const bf16_t*)in + elem);
        lo = p[0];
        hi = p[1];
    }
}

// A workgroup (4 waves) owns 128 output pixels x BN output channels.  BN = 64: each wave 32 x 64 (2 x 4 MFMA tiles), two LDS buffers and
// one barrier per K tile.  BN = 128 (Cout % 128 == 0): the waves form 2 x 2, each 64 x 64 (4 x 4 tiles: half the LDS reads per MFMA), ONE
// LDS buffer (two would pass the 64 KiB of static LDS) and two barriers per K tile, the next tile's global loads in flight across the
// compute.  Same K order: the two forms give the same bits.  Waves per SIMD: the LDS admits two workgroups of the 64 form, and the 128
// form is held to the register budget of three (without the bound the allocator settles for two).
template <int IN_F32, int OUT16, int BN>
__global__ __launch_bounds__(256, BN == 128 ? 3 : 1) void conv_mfma_kernel(const md_conv_t p) {
    constexpr int NBUF = BN == 128 ? 1 : 2, NB = BN / 64, WI = BN == 128 ? 4 : 2;
    __shared__ __attribute__((aligned(16))) bf16_t As[NBUF][CBM * CLD];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[NBUF][BN * CLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const long m0 = (long)blockIdx.x * CBM;
    const int co0 = blockIdx.y * BN;
    const int wr0 = BN == 128 ? (wave & 1) * 64 : wave * 32, wc0 = BN == 128 ? (wave >> 1) * 64 : 0;      // the wave's corner in the tile
    const int Hb = p.Hb, Wb = p.Wb, Hs = p.Hs, Ws = p.Ws, Cin = p.Cin, kw = p.kw, Ktot = p.Ktot, up2 = p.up2;
    const int nk = (Ktot + CBK - 1) / CBK;

    // staging role: rows srow and srow + 64 of the A tile, row srow (and srow + 64: BN = 128) of the B tile, the granule at kq of every K tile
    const int srow = tid >> 2, kq = (tid & 3) * 16;
    int pn[2], py[2], px[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long m = m0 + srow + 64 * t;
        const bool pv = m < p.M;
        const int mm = pv ? (int)m : 0, hw = p.Ho * p.Wo;
        pn[t] = mm / hw * Hs;                             // the sample's first source row
        const int rem = mm % hw;
        py[t] = pv ? (rem / p.Wo) * p.st - p.ph : -(1 << 30);      // the logical input row / column of tap (0, 0); a row past M lies above every image
        px[t] = (rem % p.Wo) * p.st - p.pw;
    }

    const bf16_t* wrow[NB];                               // the staged weight rows
    bool bv[NB];                                          // (inside Cout)
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int co = co0 + srow + 64 * t;
        bv[t] = co < p.Cout;
        wrow[t] = p.w + (size_t)(bv[t] ? co : 0) * Ktot;
    }

    uint4 ra[2][2], rb[NB][2];
    auto fetch = [&](int kt) {
        const int k0 = kt * CBK + kq;
        const bool kv = k0 < Ktot;                         // (Ktot % 16 == 0: a granule is inside K or past it, never across)
        const int tap = kv ? k0 / Cin : 0, c0 = kv ? k0 - tap * Cin : 0;
        const int ky = tap / kw, kx = tap - ky * kw;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int yy = py[t] + ky, xx = px[t] + kx;
            ra[t][0] = uint4{0u, 0u, 0u, 0u};
            ra[t][1] = uint4{0u, 0u, 0u, 0u};
            if (kv && yy >= 0 && yy < Hb && xx >= 0 && xx < Wb)       // (the source has fewer than 2^31 pixels: the launcher sees to it)
                load16<IN_F32>(p.in, (size_t)((pn[t] + (yy >> up2)) * Ws + (xx >> up2)) * Cin + c0, ra[t][0], ra[t][1]);
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            rb[t][0] = uint4{0u, 0u, 0u, 0u};
            rb[t][1] = uint4{0u, 0u, 0u, 0u};
            if (kv && bv[t]) {
                const uint4* wp = (const uint4*)(wrow[t] + k0);
                rb[t][0] = wp[0];
                rb[t][1] = wp[1];
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            uint4* d = (uint4*)(&As[buf][(srow + 64 * t) * CLD + kq]);
            d[0] = ra[t][0];
            d[1] = ra[t][1];
        }
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            uint4* d = (uint4*)(&Bs[buf][(srow + 64 * t) * CLD + kq]);
            d[0] = rb[t][0];
            d[1] = rb[t][1];
        }
    };

    f32x4_t acc[WI][4];
#pragma unroll
    for (int i = 0; i < WI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stash(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = NBUF == 2 ? kt & 1 : 0;
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int ks = 0; ks < CBK / 32; ++ks) {
            bf16x8_t a[WI], b[4];
#pragma unroll
            for (int i = 0; i < WI; ++i) a[i] = *(const bf16x8_t*)(&As[buf][(wr0 + i * 16 + r) * CLD + ks * 32 + q * 8]);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const bf16x8_t*)(&Bs[buf][(wc0 + j * 16 + r) * CLD + ks * 32 + q * 8]);
#pragma unroll
            for (int i = 0; i < WI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(a[i], b[j], acc[i][j]);
        }
        if constexpr (NBUF == 1) __syncthreads();       // one buffer: every wave has read K tile kt before it is overwritten
        // (two buffers: the other one was last read by the compute of K tile kt - 1, which every wave left before the previous barrier)
        if (kt + 1 < nk) stash(NBUF == 2 ? buf ^ 1 : 0);
        __syncthreads();
    }

    // accumulator element e of a lane: pixel row 4 q + e of the 16 x 16 tile, output channel r.  The residual is decided once per
    // workgroup, not per element.
    auto epilogue = [&](auto with_res) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = co0 + wc0 + j * 16 + r;
            if (co >= p.Cout) continue;
            const float bv = p.bias[co];
#pragma unroll
            for (int i = 0; i < WI; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long m = m0 + wr0 + i * 16 + q * 4 + e;
                    if (m >= p.M) continue;
                    const size_t o = (size_t)m * p.ld + p.coff + co;
                    float v = acc[i][j][e] + bv;
                    if constexpr (decltype(with_res)::value) v += p.res[o];
                    if (p.relu) v = v > 0.f ? v : 0.f;
                    if constexpr (OUT16) ((bf16_t*)p.out)[o] = cvt16s(v);
                    else ((float*)p.out)[o] = v;
                }
        }
    };
    if (p.res) epilogue(std::true_type{});
    else epilogue(std::false_type{});
}

// Every other shape (K = 27 or 36 first layers, 3 outputs with an NCHW store, 4 -> 4 from NCHW) and every misaligned operand: one
// thread per output element, the same operand rounding, a serial fp32 sum in (ky, kx, c) order.
template <int IN_KIND> __global__ __launch_bounds__(256) void conv_plain_kernel(const md_conv_t p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.M * p.Cout) return;
    const int co = (int)(idx % p.Cout);
    const long m = idx / p.Cout;
    const int Hb = p.Hb, Wb = p.Wb, Hs = p.Hs, Ws = p.Ws, Cin = p.Cin, hw = p.Ho * p.Wo;
    const int n = (int)(m / hw), rem = (int)(m % hw), y = rem / p.Wo, x = rem % p.Wo;
    const bf16_t* wr = p.w + (size_t)co * p.Ktot;
    float acc = 0.f;
    for (int ky = 0; ky < p.kh; ++ky) {
        const int yy = y * p.st + ky - p.ph;
        if (yy < 0 || yy >= Hb) continue;
        for (int kx = 0; kx < p.kw; ++kx) {
            const int xx = x * p.st + kx - p.pw;
            if (xx < 0 || xx >= Wb) continue;
            const int ys = yy >> p.up2, xs = xx >> p.up2;
            const bf16_t* wt = wr + (size_t)(ky * p.kw + kx) * Cin;
            if constexpr (IN_KIND == MAPDIT_VAE_IN_16) {
                const bf16_t* ip = (const bf16_t*)p.in + (((size_t)n * Hs + ys) * Ws + xs) * Cin;
                int c = 0;
                if (Cin % 8 == 0 && !(((uintptr_t)ip | (uintptr_t)wt) & 15))        // eight channels per 16-byte load, the same serial order
                    for (; c < Cin; c += 8) {
                        const uint4 xv = *(const uint4*)(ip + c), wv = *(const uint4*)(wt + c);
                        const uint32_t xw[4] = {xv.x, xv.y, xv.z, xv.w}, ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc = fmaf(lo16(xw[e]), lo16(ww[e]), acc);
                            acc = fmaf(hi16(xw[e]), hi16(ww[e]), acc);
                        }
                    }
                for (; c < Cin; ++c) acc = fmaf(up16(ip[c]), up16(wt[c]), acc);
            } else if constexpr (IN_KIND == MAPDIT_VAE_IN_F32) {
                const float* ip = (const float*)p.in + (((size_t)n * Hs + ys) * Ws + xs) * Cin;
                for (int c = 0; c < Cin; ++c) acc = fmaf(up16(cvt16s(ip[c])), up16(wt[c]), acc);
            } else {
                const float* ip = (const float*)p.in + ((size_t)n * Cin * Hs + ys) * Ws + xs;
                for (int c = 0; c < Cin; ++c) acc = fmaf(up16(cvt16s(ip[(size_t)c * Hs * Ws])), up16(wt[c]), acc);
            }
        }
    }
    const bool nchw = p.out_kind == MAPDIT_VAE_OUT_F32_NCHW;      // (dense, no residual: the launcher sees to it)
    const size_t o = nchw ? (((size_t)n * p.Cout + co) * p.Ho + y) * p.Wo + x : (size_t)m * p.ld + p.coff + co;
    float v = acc + p.bias[co];
    if (p.res) v += p.res[o];
    if (p.relu) v = v > 0.f ? v : 0.f;
    if (p.out_kind == MAPDIT_VAE_OUT_16) ((bf16_t*)p.out)[o] = cvt16s(v);
    else ((float*)p.out)[o] = v;
}

MD_NS_CLOSE

// The caller chooses the tile (the choice decides the bits, so it stays the entry point's); a tile whose preconditions do not hold is
// refused here, never replaced by another.
int MD_SYM(conv_launch)(const char* who, const md_conv_t* pp, int tile, void* stream) {
    const md_conv_t& p = *pp;
    hipStream_t st = (hipStream_t)stream;
    const bool nchw = p.in_kind == MAPDIT_VAE_IN_F32_NCHW || p.out_kind == MAPDIT_VAE_OUT_F32_NCHW;
    MD_CHECK(p.M > 0, "%s: empty output", who);
    MD_CHECK(p.M < (1L << 31) && (long)p.M * p.ld < (1L << 40), "%s: %ld output pixels are too many", who, p.M);
    const long K = (long)p.kh * p.kw * p.Cin;
    MD_CHECK(K == p.Ktot && K < (1L << 24), "%s: K = %ld is too long", who, K);
    MD_CHECK(p.out_kind != MAPDIT_VAE_OUT_F32_NCHW || (!p.res && p.ld == p.Cout && p.coff == 0), "%s: the NCHW store is dense and takes no residual", who);
    if (tile == MD_CONV_PLAIN) {
        MD_CHECK(p.M * p.Cout < (1L << 38), "%s: %ld x %d outputs are too many for the plain kernel", who, p.M, p.Cout);
        const int grid = cdiv(p.M * p.Cout, 256);
        if (p.in_kind == MAPDIT_VAE_IN_16) conv_plain_kernel<MAPDIT_VAE_IN_16><<<grid, 256, 0, st>>>(p);
        else if (p.in_kind == MAPDIT_VAE_IN_F32) conv_plain_kernel<MAPDIT_VAE_IN_F32><<<grid, 256, 0, st>>>(p);
        else conv_plain_kernel<MAPDIT_VAE_IN_F32_NCHW><<<grid, 256, 0, st>>>(p);
    } else {
        MD_CHECK(tile == MD_CONV_64 || tile == MD_CONV_128, "%s: no convolution tile %d", who, tile);
        const long src = p.M / ((long)p.Ho * p.Wo) * p.Hs * p.Ws;      // the MFMA gather indexes source pixels in 32 bits
        MD_CHECK(src < (1L << 31), "%s: %ld input pixels are too many", who, src);
        MD_CHECK(!(((uintptr_t)p.in | (uintptr_t)p.w) & 15) && p.Cin % 16 == 0 && p.Cout % 16 == 0 && !nchw && (tile == MD_CONV_64 || p.Cout % 128 == 0),
                 "%s: the %d-wide MFMA tile needs 16-byte aligned NHWC operands, Cin %% 16 == 0 and Cout %% %d == 0 (Cin=%d, Cout=%d)", who, tile,
                 tile == MD_CONV_128 ? 128 : 16, p.Cin, p.Cout);
        const bool f32 = p.in_kind == MAPDIT_VAE_IN_F32, o16 = p.out_kind == MAPDIT_VAE_OUT_16;
        const dim3 grid((unsigned)cdiv(p.M, CBM), (unsigned)cdiv(p.Cout, tile));
#define CONV_GO(F, O)                                                              \
    do {                                                                           \
        if (tile == MD_CONV_128) conv_mfma_kernel<F, O, 128><<<grid, 256, 0, st>>>(p); \
        else conv_mfma_kernel<F, O, 64><<<grid, 256, 0, st>>>(p);                  \
    } while (0)
        if (f32 && o16) CONV_GO(1, 1);
        else if (f32) CONV_GO(1, 0);
        else if (o16) CONV_GO(0, 1);
        else CONV_GO(0, 0);
#undef CONV_GO
    }
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
