// Sample-quality metrics on feature sets (metrics.py: precision / recall, density / coverage, KID): the Gram matrix G = R Q^T of two
// row-major fp32 sets [rows, D], computed tile by tile on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding
// per step of the chain) and never stored.  Every 128 x 128 tile is reduced in the epilogue to what the metric needs - the 8 smallest
// squared distances per query, a count of references whose ball holds the query, an fp64 sum of polynomial-kernel values, or the
// softmax statistics of the Inception Score (mapdit_softmax_score: the Gram values are logits; per sample an online (max, sum exp,
// sum exp * logit) over the classes, then with the roles swapped per class the sum of exp(logit - lse) over the samples - fp32 ends
// at the Gram value, the bias, exp and log are fp64).  One kernel, five epilogues (the template argument).  fp32 only: built once,
// not per 16-bit operand format.
//
// Tile: 128 references (the MFMA's A side, the rows of C) x 128 queries (B side, the columns of C) x 32 of K, 4 waves, each 2 x 2 tiles
// of 32 x 32.  In the 32 x 32 C layout a lane owns ONE column and 16 rows, so with the queries on the columns a lane reduces over
// its own references in registers; the two lane halves and the two waves that share a query meet in LDS once, at the end of the
// workgroup.  Both operands are K-contiguous: staged through registers (the next K tile is in flight while this one is multiplied)
// into LDS rows padded to 36 floats, read back as one float4 of K per lane.  A lane half h therefore feeds k = 8 s + 4 h + j to step
// j of read s: the K order of the chain is a fixed permutation, the same for every element, so G(i, j) == G(j, i) bit for bit.
//
// Grid: query tiles x `chunks` slices of the reference tiles.  Partial results go to the workspace and a small second kernel merges
// them: a k-smallest set, an integer count and a sum over per-tile partials in a fixed order do not depend on the slicing.  No atomics.
// The softmax epilogues keep that promise the way MF_POLY does: one (m, s, u) per (sample, class tile) and one fp64 sum per (class,
// sample tile, wave), merged in tile order - every output of mapdit_softmax_score is independent of `chunks` bit for bit.
#include <type_traits>

#include "common.h"

namespace {

constexpr int MF_TILE = 128, MF_BK = 32, MF_LD = 36, MF_THREADS = 256, MF_KMAX = 8;
constexpr int MF_MAX_ROWS = 1 << 30;        // row indices, tile counts and rows + 127 stay in int; row offsets are 64-bit
constexpr int MF_MAX_D = 65536, MF_MAX_CHUNKS = 65535;
enum { MF_KNN = 0, MF_COUNT = 1, MF_POLY = 2, MF_LSE = 3, MF_MARGINAL = 4 };

struct mf_args_t {
    const float* Q;           // [Nq, D] queries: the columns of a tile
    const float* R;           // [Nr, D] references: the rows
    int Nq, Nr, D;
    const float* nq;          // squared row norms (KNN, COUNT)
    const float* nr;
    const float* rad;         // COUNT: [Nr] (MAPDIT_BALL_REF_RADIUS) or [Nq] (MAPDIT_BALL_QUERY_RADIUS)
    int mode, self;           // self: the pair (q, r) with q == r by index is skipped
    double gamma, coef0;      // POLY
    int degree;
    int chunks, rtiles;
    float* knn_part;          // [chunks][Nq][8] ascending
    uint32_t* cnt_part;       // [chunks][Nq]
    double* sum_part;         // [qtiles][rtiles][4 waves]
    const float* bias;        // LSE: [Nr] (the classes are the references), MARGINAL: [Nq]; or null
    const double* lse;        // MARGINAL: [Nr], each sample's log-sum-exp
    double* lse_part;         // LSE: [rtiles][Nq][3] = (m, s, u) of a sample over one class tile
    double* marg_part;        // MARGINAL: [rtiles][Nq][2 waves]
};

// (m, s, u) = (max l, sum exp(l - m), sum exp(l - m) l) of two disjoint sets of logits; (-inf, 0, 0) is the empty set
__device__ __forceinline__ void mf_lse_merge(double& m, double& s, double& u, double m2, double s2, double u2) {
    const double mn = fmax(m, m2);
    if (mn == -__builtin_inf()) return;
    const double a = exp(m - mn), b = exp(m2 - mn);
    s = s * a + s2 * b;
    u = u * a + u2 * b;
    m = mn;
}

// the 8 smallest of a stream, ascending: one compare-exchange per slot
__device__ __forceinline__ void mf_insert(float (&lst)[MF_KMAX], float d) {
#pragma unroll
    for (int t = 0; t < MF_KMAX; ++t) {
        const float lo = fminf(lst[t], d);
        d = fmaxf(lst[t], d);
        lst[t] = lo;
    }
}

template <int EPI>
__global__ __launch_bounds__(MF_THREADS, 2) void gram_tile_kernel(mf_args_t p) {
    __shared__ __attribute__((aligned(16))) float sR[MF_TILE * MF_LD];
    __shared__ __attribute__((aligned(16))) float sQ[MF_TILE * MF_LD];
    __shared__ float sNr[MF_TILE], sRad[MF_TILE];
    __shared__ double sLse[MF_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, l31 = lane & 31, half = lane >> 5;
    const int qtile = blockIdx.x, chunk = blockIdx.y;
    const int q0 = qtile * MF_TILE;
    const int rt_begin = (int)((long)chunk * p.rtiles / p.chunks), rt_end = (int)((long)(chunk + 1) * p.rtiles / p.chunks);
    const int nk = (p.D + MF_BK - 1) / MF_BK;

    // staging: thread t moves the float4 at K column 4 (t % 8) of rows t / 8 + 32 i; rows past the end re-read the last row (masked below)
    const int ld_row = tid >> 3, ld_col = (tid & 7) * 4;
    const float* qsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qsrc[i] = p.Q + (size_t)min(q0 + ld_row + 32 * i, p.Nq - 1) * p.D + ld_col;

    int qidx[2];
    float nqv[2], radq[2], biasq[2];
    float lst[2][MF_KMAX];
    uint32_t cnt[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        qidx[n] = q0 + wn * 64 + n * 32 + l31;
        const bool in = qidx[n] < p.Nq;
        nqv[n] = ((EPI == MF_KNN || EPI == MF_COUNT) && in) ? p.nq[qidx[n]] : 0.f;
        biasq[n] = (EPI == MF_MARGINAL && p.bias && in) ? p.bias[qidx[n]] : 0.f;
        radq[n] = (EPI == MF_COUNT && p.mode == MAPDIT_BALL_QUERY_RADIUS && in) ? p.rad[qidx[n]] : 0.f;
        cnt[n] = 0;
#pragma unroll
        for (int t = 0; t < MF_KMAX; ++t) lst[n][t] = __builtin_inff();
    }

    for (int rt = rt_begin; rt < rt_end; ++rt) {
        const int r0 = rt * MF_TILE;
        const float* rsrc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rsrc[i] = p.R + (size_t)min(r0 + ld_row + 32 * i, p.Nr - 1) * p.D + ld_col;
        f32x16_t acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

        float4 gr[4], gq[4];
        auto fetch = [&](int kt) {
            const int k = kt * MF_BK;
            const bool in = k + ld_col < p.D;                  // D % 4 == 0: a float4 lies inside or outside as a whole
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gr[i] = in ? *reinterpret_cast<const float4*>(rsrc[i] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
                gq[i] = in ? *reinterpret_cast<const float4*>(qsrc[i] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        fetch(0);
        for (int kt = 0; kt < nk; ++kt) {
            __syncthreads();                                   // the previous K tile (and the previous epilogue's sNr / sRad) is read
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<float4*>(&sR[(ld_row + 32 * i) * MF_LD + ld_col]) = gr[i];
                *reinterpret_cast<float4*>(&sQ[(ld_row + 32 * i) * MF_LD + ld_col]) = gq[i];
            }
            if ((EPI == MF_LSE || EPI == MF_MARGINAL) && kt == 0 && tid < MF_TILE) {
                const bool in = r0 + tid < p.Nr;
                if (EPI == MF_LSE) sNr[tid] = (in && p.bias) ? p.bias[r0 + tid] : 0.f;
                else sLse[tid] = in ? p.lse[r0 + tid] : 0.0;
            }
            if ((EPI == MF_KNN || EPI == MF_COUNT) && kt == 0 && tid < MF_TILE) {
                const bool in = r0 + tid < p.Nr;
                sNr[tid] = in ? p.nr[r0 + tid] : 0.f;
                if (EPI == MF_COUNT) sRad[tid] = (in && p.mode == MAPDIT_BALL_REF_RADIUS) ? p.rad[r0 + tid] : 0.f;
            }
            __syncthreads();
            if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
            for (int s = 0; s < MF_BK / 8; ++s) {
                float4 a[2], b[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const float4*>(&sR[(wm * 64 + m * 32 + l31) * MF_LD + s * 8 + half * 4]);
#pragma unroll
                for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const float4*>(&sQ[(wn * 64 + n * 32 + l31) * MF_LD + s * 8 + half * 4]);
                const float av[2][4] = {{a[0].x, a[0].y, a[0].z, a[0].w}, {a[1].x, a[1].y, a[1].z, a[1].w}};
                const float bv[2][4] = {{b[0].x, b[0].y, b[0].z, b[0].w}, {b[1].x, b[1].y, b[1].z, b[1].w}};
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][j], bv[n][j], acc[m][n], 0, 0, 0);
            }
        }

        // epilogue: C element r of a lane is row (r & 3) + 8 (r >> 2) + 4 half (a reference), column lane & 31 (a query)
        // (the polynomial's degree is a compile-time constant of the element loop: one uniform switch per tile, not a loop per element)
        double tsum = 0.0;
        auto reduce_tile = [&](auto degree) {
            constexpr int DEG = decltype(degree)::value;
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        const int ridx = r0 + lr;
                        const float g = acc[m][n][r];
                        const bool valid = ridx < p.Nr && !(p.self && ridx == qidx[n]);
                        if (EPI == MF_POLY) {
                            const double v = p.gamma * (double)g + p.coef0;
                            double pw = v;
#pragma unroll
                            for (int e = 1; e < DEG; ++e) pw *= v;
                            tsum += (valid && qidx[n] < p.Nq) ? pw : 0.0;
                        } else {
                            const float d = fmaxf(0.f, fmaf(-2.f, g, nqv[n] + sNr[lr]));
                            if (EPI == MF_KNN) {
                                if (valid && d < lst[n][MF_KMAX - 1]) mf_insert(lst[n], d);
                            } else {
                                const float thr = p.mode == MAPDIT_BALL_REF_RADIUS ? sRad[lr] : radq[n];
                                cnt[n] += (valid && d <= thr) ? 1u : 0u;
                            }
                        }
                    }
        };
        if constexpr (EPI == MF_LSE) {
            // fp32 ends at g: the logit l = g + bias and everything after it is fp64.  A lane's 32 classes of the tile per query in
            // two blocks of 16 (one accumulator each: 16 logits are live at a time, not 64), merged in block order; then the four
            // lanes that hold the same query (slot = 2 wm + half) meet in LDS and merge in slot order: one partial per (sample, class
            // tile), whatever the slicing
            double pm[2], ps[2], pu[2];
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                pm[n] = -__builtin_inf();
                ps[n] = pu[n] = 0.0;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    double l[16], mx = -__builtin_inf();
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        l[r] = (r0 + lr < p.Nr) ? (double)acc[m][n][r] + (double)sNr[lr] : -__builtin_inf();
                        mx = fmax(mx, l[r]);
                    }
                    double s = 0.0, u = 0.0;
                    if (mx != -__builtin_inf()) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const bool in = l[r] != -__builtin_inf();          // (rows past the end: exp(-inf) = 0, but 0 * -inf is no 0)
                            const double e = in ? exp(l[r] - mx) : 0.0;
                            s += e;
                            u += in ? e * l[r] : 0.0;
                        }
                    }
                    mf_lse_merge(pm[n], ps[n], pu[n], mx, s, u);
                    __builtin_amdgcn_sched_barrier(0);         // block by block: the next block's logits are not formed ahead of time
                }
            }
            __syncthreads();                                   // every wave is done with sR: it becomes [128 queries][4 slots][3] doubles, 12 KB
            double* mb = reinterpret_cast<double*>(sR);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                double* d = mb + ((wn * 64 + n * 32 + l31) * 4 + 2 * wm + half) * 3;
                d[0] = pm[n];
                d[1] = ps[n];
                d[2] = pu[n];
            }
            __syncthreads();
            if (tid < MF_TILE && q0 + tid < p.Nq) {
                double m = mb[tid * 12], s = mb[tid * 12 + 1], u = mb[tid * 12 + 2];
                for (int t = 1; t < 4; ++t) mf_lse_merge(m, s, u, mb[tid * 12 + 3 * t], mb[tid * 12 + 3 * t + 1], mb[tid * 12 + 3 * t + 2]);
                double* dst = p.lse_part + ((size_t)rt * p.Nq + q0 + tid) * 3;
                dst[0] = m;
                dst[1] = s;
                dst[2] = u;
            }                                                  // (the next tile's first barrier comes before sR is written again)
        } else if constexpr (EPI == MF_MARGINAL) {
            // the same logit bits with the roles swapped (g is symmetric): exp(l - lse) of a lane's 32 samples per class, the two lane
            // halves by one exchange (a + b == b + a), one partial per (class, sample tile) and wave
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        const double l = (double)acc[m][n][r] + (double)biasq[n];
                        s += (r0 + lr < p.Nr) ? exp(l - sLse[lr]) : 0.0;
                    }
                s += __shfl_xor(s, 32, 64);
                if (half == 0 && qidx[n] < p.Nq) p.marg_part[((size_t)rt * p.Nq + qidx[n]) * 2 + wm] = s;
            }
        } else if (EPI != MF_POLY || p.degree == 1) reduce_tile(std::integral_constant<int, 1>{});
        else if (p.degree == 2) reduce_tile(std::integral_constant<int, 2>{});
        else if (p.degree == 3) reduce_tile(std::integral_constant<int, 3>{});
        else reduce_tile(std::integral_constant<int, 4>{});
        if (EPI == MF_POLY) {
            // one partial per (query tile, reference tile, wave): the butterfly gives every lane the same bits
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) tsum += __shfl_xor(tsum, o, 64);
            if (lane == 0) p.sum_part[((size_t)qtile * p.rtiles + rt) * 4 + wave] = tsum;
        }
    }

    if (EPI == MF_POLY || EPI == MF_LSE || EPI == MF_MARGINAL) return;
    // the two lane halves and the two waves (wm) that hold the same query meet here: slot = 2 wm + half
    __syncthreads();
    const int ql = wn * 64 + l31, slot = 2 * wm + half;
    if (EPI == MF_KNN) {
        float* mb = sR;                                        // [128 queries][4 slots][8]: 16 KB of sR's 18
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int t = 0; t < MF_KMAX; ++t) mb[((ql + n * 32) * 4 + slot) * MF_KMAX + t] = lst[n][t];
        __syncthreads();
        if (tid < MF_TILE && q0 + tid < p.Nq) {
            float out[MF_KMAX];
#pragma unroll
            for (int t = 0; t < MF_KMAX; ++t) out[t] = mb[(tid * 4) * MF_KMAX + t];
            for (int s = 1; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < MF_KMAX; ++t) mf_insert(out, mb[(tid * 4 + s) * MF_KMAX + t]);
            float* dst = p.knn_part + ((size_t)chunk * p.Nq + q0 + tid) * MF_KMAX;
#pragma unroll
            for (int t = 0; t < MF_KMAX; ++t) dst[t] = out[t];
        }
    } else {
        uint32_t* mb = reinterpret_cast<uint32_t*>(sR);        // [128 queries][4 slots]
#pragma unroll
        for (int n = 0; n < 2; ++n) mb[(ql + n * 32) * 4 + slot] = cnt[n];
        __syncthreads();
        if (tid < MF_TILE && q0 + tid < p.Nq)
            p.cnt_part[(size_t)chunk * p.Nq + q0 + tid] = mb[tid * 4] + mb[tid * 4 + 1] + mb[tid * 4 + 2] + mb[tid * 4 + 3];
    }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part, int N, int chunks, int k, float* __restrict__ radii) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    float lst[MF_KMAX];
#pragma unroll
    for (int t = 0; t < MF_KMAX; ++t) lst[t] = __builtin_inff();
    for (int c = 0; c < chunks; ++c) {
        const float* src = part + ((size_t)c * N + q) * MF_KMAX;
#pragma unroll
        for (int t = 0; t < MF_KMAX; ++t) mf_insert(lst, src[t]);
    }
    float out = lst[0];
#pragma unroll
    for (int t = 1; t < MF_KMAX; ++t) out = (t == k - 1) ? lst[t] : out;
    radii[q] = out;
}

__global__ __launch_bounds__(256) void count_merge_kernel(const uint32_t* __restrict__ part, int N, int chunks, uint32_t* __restrict__ count) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    uint32_t s = 0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * N + q];
    count[q] = s;
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void sum_merge_kernel(const double* __restrict__ part, size_t n, double* __restrict__ out) {
    __shared__ double s[256];
    double v = 0.0;
    for (size_t i = threadIdx.x; i < n; i += 256) v += part[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// one thread per sample: the class tiles' (m, s, u) in tile order -> lse = m + log s and sum_c p log p = u / s - lse
__global__ __launch_bounds__(256) void lse_merge_kernel(const double* __restrict__ part, int N, int rtiles, double* __restrict__ lse,
                                                        double* __restrict__ plogp) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    double m = -__builtin_inf(), s = 0.0, u = 0.0;
    for (int rt = 0; rt < rtiles; ++rt) {
        const double* src = part + ((size_t)rt * N + q) * 3;
        mf_lse_merge(m, s, u, src[0], src[1], src[2]);
    }
    const double l = m + log(s);
    lse[q] = l;
    plogp[q] = u / s - l;
}

// one thread per class: the (sample tile, wave) partials in index order
__global__ __launch_bounds__(256) void marg_merge_kernel(const double* __restrict__ part, int C, int rtiles, double* __restrict__ marg) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double v = 0.0;
    for (int rt = 0; rt < rtiles; ++rt) {
        v += part[((size_t)rt * C + c) * 2];
        v += part[((size_t)rt * C + c) * 2 + 1];
    }
    marg[c] = v;
}

// one wave per row: lane l adds the float4s l, l + 64, ... of the row in fp64, then the butterfly; one rounding to fp32 at the end
__global__ __launch_bounds__(256) void row_sqnorm_kernel(const float* __restrict__ X, int N, int D, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* x = X + (size_t)row * D;
    double s = 0.0;
    for (int k = lane * 4; k < D; k += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + k);
        s += (double)v.x * v.x;
        s += (double)v.y * v.y;
        s += (double)v.z * v.z;
        s += (double)v.w * v.w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = (float)s;
}

bool mf_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

int mf_tiles(int rows) { return (rows + MF_TILE - 1) / MF_TILE; }

// the slice count: a forced one as given (slices beyond the reference tiles are empty and merge as nothing), or enough to give
// the chip's 256 CUs two workgroups each
int mf_chunks(int qtiles, int rtiles, int chunks) {
    if (chunks > 0) return chunks;
    const int want = (512 + qtiles - 1) / qtiles;
    return want < 1 ? 1 : want > rtiles ? rtiles : want;
}

int mf_check_ptr(const char* who, const char* name, const float* X) {
    MD_CHECK(mf_aligned(X, 16), "%s: %s is null or not 16-byte aligned", who, name);
    return MAPDIT_OK;
}

int mf_check_shape(const char* who, int Nq, int Nr, int D, int chunks) {
    MD_CHECK(D >= 4 && D % 4 == 0 && D <= MF_MAX_D, "%s: D=%d (a multiple of 4, at most %d: rows are read as float4)", who, D, MF_MAX_D);
    MD_CHECK(Nq >= 1 && Nq <= MF_MAX_ROWS && Nr >= 1 && Nr <= MF_MAX_ROWS, "%s: %d x %d rows (1 .. 2^30 each: row indices are 32-bit)", who, Nq, Nr);
    MD_CHECK(chunks >= 0 && chunks <= MF_MAX_CHUNKS, "%s: chunks=%d (0 = chosen by the library, at most %d)", who, chunks, MF_MAX_CHUNKS);
    return MAPDIT_OK;
}

size_t mf_norm_bytes(int N) { return md_up256((size_t)N * sizeof(float)); }

template <int EPI>
int mf_launch(const mf_args_t& a, void* stream) {
    hipLaunchKernelGGL(gram_tile_kernel<EPI>, dim3((unsigned)mf_tiles(a.Nq), (unsigned)a.chunks), dim3(MF_THREADS), 0, (hipStream_t)stream, a);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

int mf_sqnorm(const float* X, int N, int D, float* out, void* stream) {
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, X, N, D, out);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

}  // namespace

extern "C" int mapdit_row_sqnorm(const float* X, int N, int D, float* out, void* stream) {
    MD_TRY(mf_check_shape("row_sqnorm", N, N, D, 0));
    MD_TRY(mf_check_ptr("row_sqnorm", "X", X));
    MD_CHECK(mf_aligned(out, 4), "row_sqnorm: out is null or unaligned");
    return mf_sqnorm(X, N, D, out, stream);
}

extern "C" size_t mapdit_knn_radii_workspace_bytes(int N, int D, int chunks) {
    if (mf_check_shape("knn_radii", N, N, D, chunks) != MAPDIT_OK) return 0;
    const int c = mf_chunks(mf_tiles(N), mf_tiles(N), chunks);
    return mf_norm_bytes(N) + (size_t)c * N * MF_KMAX * sizeof(float);
}

extern "C" int mapdit_knn_radii(const float* X, int N, int D, int k, float* radii, int chunks, void* workspace, size_t ws_bytes, void* stream) {
    MD_TRY(mf_check_shape("knn_radii", N, N, D, chunks));
    MD_TRY(mf_check_ptr("knn_radii", "X", X));
    MD_CHECK(k >= 1 && k <= MF_KMAX, "knn_radii: k=%d (1 .. %d)", k, MF_KMAX);
    MD_CHECK(k < N, "knn_radii: k=%d needs more than %d rows (a row is not its own neighbour)", k, N);
    MD_CHECK(mf_aligned(radii, 4), "knn_radii: radii is null or unaligned");
    const size_t need = mapdit_knn_radii_workspace_bytes(N, D, chunks);
    MD_CHECK(mf_aligned(workspace, 256) && ws_bytes >= need, "knn_radii: workspace of %zu bytes at %p (%zu needed, 256-byte aligned)", ws_bytes,
             workspace, need);
    mf_args_t a = {};
    float* norms = (float*)workspace;
    a.Q = a.R = X;
    a.Nq = a.Nr = N;
    a.D = D;
    a.nq = a.nr = norms;
    a.self = 1;
    a.rtiles = mf_tiles(N);
    a.chunks = mf_chunks(mf_tiles(N), a.rtiles, chunks);
    a.knn_part = (float*)((char*)workspace + mf_norm_bytes(N));
    MD_TRY(mf_sqnorm(X, N, D, norms, stream));
    MD_TRY(mf_launch<MF_KNN>(a, stream));
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a.knn_part, N, a.chunks, k, radii);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" size_t mapdit_ball_count_workspace_bytes(int Nq, int Nr, int D, int chunks) {
    if (mf_check_shape("ball_count", Nq, Nr, D, chunks) != MAPDIT_OK) return 0;
    const int c = mf_chunks(mf_tiles(Nq), mf_tiles(Nr), chunks);
    return mf_norm_bytes(Nq) + mf_norm_bytes(Nr) + (size_t)c * Nq * sizeof(uint32_t);
}

extern "C" int mapdit_ball_count(const float* Q, int Nq, const float* R, int Nr, int D, const float* rad, int mode, int self, uint32_t* count,
                                 int chunks, void* workspace, size_t ws_bytes, void* stream) {
    MD_TRY(mf_check_shape("ball_count", Nq, Nr, D, chunks));
    MD_TRY(mf_check_ptr("ball_count", "Q", Q));
    MD_TRY(mf_check_ptr("ball_count", "R", R));
    MD_CHECK(mode == MAPDIT_BALL_REF_RADIUS || mode == MAPDIT_BALL_QUERY_RADIUS, "ball_count: mode=%d (MAPDIT_BALL_REF_RADIUS or _QUERY_RADIUS)", mode);
    MD_CHECK(self == 0 || (self == 1 && Q == R && Nq == Nr), "ball_count: self=%d skips q == r, which needs Q == R (and 0 or 1)", self);
    MD_CHECK(mf_aligned(rad, 4) && mf_aligned(count, 4), "ball_count: rad or count is null or unaligned");
    const size_t need = mapdit_ball_count_workspace_bytes(Nq, Nr, D, chunks);
    MD_CHECK(mf_aligned(workspace, 256) && ws_bytes >= need, "ball_count: workspace of %zu bytes at %p (%zu needed, 256-byte aligned)", ws_bytes,
             workspace, need);
    mf_args_t a = {};
    float* nq = (float*)workspace;
    float* nr = (float*)((char*)workspace + mf_norm_bytes(Nq));
    a.Q = Q;
    a.R = R;
    a.Nq = Nq;
    a.Nr = Nr;
    a.D = D;
    a.nq = nq;
    a.nr = nr;
    a.rad = rad;
    a.mode = mode;
    a.self = self;
    a.rtiles = mf_tiles(Nr);
    a.chunks = mf_chunks(mf_tiles(Nq), a.rtiles, chunks);
    a.cnt_part = (uint32_t*)((char*)workspace + mf_norm_bytes(Nq) + mf_norm_bytes(Nr));
    MD_TRY(mf_sqnorm(Q, Nq, D, nq, stream));
    MD_TRY(mf_sqnorm(R, Nr, D, nr, stream));
    MD_TRY(mf_launch<MF_COUNT>(a, stream));
    hipLaunchKernelGGL(count_merge_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a.cnt_part, Nq, a.chunks, count);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

extern "C" size_t mapdit_poly_kernel_sum_workspace_bytes(int Na, int Nb, int D, int chunks) {
    if (mf_check_shape("poly_kernel_sum", Na, Nb, D, chunks) != MAPDIT_OK) return 0;
    return (size_t)mf_tiles(Na) * mf_tiles(Nb) * 4 * sizeof(double);       // (does not depend on chunks: one partial per tile pair and wave)
}

extern "C" int mapdit_poly_kernel_sum(const float* A, int Na, const float* B, int Nb, int D, double gamma, double coef0, int degree, int skip_diag,
                                      double* out, int chunks, void* workspace, size_t ws_bytes, void* stream) {
    MD_TRY(mf_check_shape("poly_kernel_sum", Na, Nb, D, chunks));
    MD_TRY(mf_check_ptr("poly_kernel_sum", "A", A));
    MD_TRY(mf_check_ptr("poly_kernel_sum", "B", B));
    MD_CHECK(degree >= 1 && degree <= 4, "poly_kernel_sum: degree=%d (1 .. 4)", degree);
    MD_CHECK(skip_diag == 0 || (skip_diag == 1 && A == B && Na == Nb), "poly_kernel_sum: skip_diag=%d drops i == j, which needs A == B (and 0 or 1)",
             skip_diag);
    MD_CHECK(mf_aligned(out, 8), "poly_kernel_sum: out is null or unaligned");
    const size_t need = mapdit_poly_kernel_sum_workspace_bytes(Na, Nb, D, chunks);
    MD_CHECK(mf_aligned(workspace, 256) && ws_bytes >= need, "poly_kernel_sum: workspace of %zu bytes at %p (%zu needed, 256-byte aligned)", ws_bytes,
             workspace, need);
    mf_args_t a = {};
    a.Q = A;
    a.R = B;
    a.Nq = Na;
    a.Nr = Nb;
    a.D = D;
    a.self = skip_diag;
    a.gamma = gamma;
    a.coef0 = coef0;
    a.degree = degree;
    a.rtiles = mf_tiles(Nb);
    a.chunks = mf_chunks(mf_tiles(Na), a.rtiles, chunks);
    a.sum_part = (double*)workspace;
    MD_TRY(mf_launch<MF_POLY>(a, stream));
    hipLaunchKernelGGL(sum_merge_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a.sum_part, (size_t)mf_tiles(Na) * a.rtiles * 4, out);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}

namespace {
struct mf_score_plan_t {
    size_t off_lse_part, off_lse, off_plogp, off_marg_part, total;
};

// does not depend on chunks: every partial belongs to a tile
mf_score_plan_t mf_score_plan(int N, int C) {
    mf_score_plan_t pl;
    size_t o = 0;
    pl.off_lse_part = o; o += md_up256((size_t)mf_tiles(C) * N * 3 * sizeof(double));
    pl.off_lse = o; o += md_up256((size_t)N * sizeof(double));
    pl.off_plogp = o; o += md_up256((size_t)N * sizeof(double));
    pl.off_marg_part = o; o += md_up256((size_t)mf_tiles(N) * C * 2 * sizeof(double));
    pl.total = o;
    return pl;
}
}  // namespace

extern "C" size_t mapdit_softmax_score_workspace_bytes(int N, int C, int D, int chunks) {
    if (mf_check_shape("softmax_score", N, C, D, chunks) != MAPDIT_OK) return 0;
    return mf_score_plan(N, C).total;
}

extern "C" int mapdit_softmax_score(const float* X, int N, const float* W, int C, int D, const float* bias, double* ent, double* marg, int chunks,
                                    void* workspace, size_t ws_bytes, void* stream) {
    MD_TRY(mf_check_shape("softmax_score", N, C, D, chunks));
    MD_TRY(mf_check_ptr("softmax_score", "X", X));
    MD_TRY(mf_check_ptr("softmax_score", "W", W));
    MD_CHECK(!bias || mf_aligned(bias, 4), "softmax_score: bias is unaligned");
    MD_CHECK(mf_aligned(ent, 8) && mf_aligned(marg, 8), "softmax_score: ent or marg is null or unaligned");
    const mf_score_plan_t pl = mf_score_plan(N, C);
    MD_CHECK(mf_aligned(workspace, 256) && ws_bytes >= pl.total, "softmax_score: workspace of %zu bytes at %p (%zu needed, 256-byte aligned)", ws_bytes,
             workspace, pl.total);
    char* ws = (char*)workspace;
    double* lse = (double*)(ws + pl.off_lse);
    double* plogp = (double*)(ws + pl.off_plogp);
    // samples as queries, classes as references: lse and sum_c p log p per sample
    mf_args_t a = {};
    a.Q = X;
    a.R = W;
    a.Nq = N;
    a.Nr = C;
    a.D = D;
    a.bias = bias;
    a.rtiles = mf_tiles(C);
    a.chunks = mf_chunks(mf_tiles(N), a.rtiles, chunks);
    a.lse_part = (double*)(ws + pl.off_lse_part);
    MD_TRY(mf_launch<MF_LSE>(a, stream));
    hipLaunchKernelGGL(lse_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a.lse_part, N, a.rtiles, lse, plogp);
    MD_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_merge_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, plogp, (size_t)N, ent);
    MD_LAUNCH_CHECK();
    // classes as queries, samples as references: the class marginal
    mf_args_t b = {};
    b.Q = W;
    b.R = X;
    b.Nq = C;
    b.Nr = N;
    b.D = D;
    b.bias = bias;
    b.lse = lse;
    b.rtiles = mf_tiles(N);
    b.chunks = mf_chunks(mf_tiles(C), b.rtiles, chunks);
    b.marg_part = (double*)(ws + pl.off_marg_part);
    MD_TRY(mf_launch<MF_MARGINAL>(b, stream));
    hipLaunchKernelGGL(marg_merge_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, b.marg_part, C, b.rtiles, marg);
    MD_LAUNCH_CHECK();
    return MAPDIT_OK;
}
