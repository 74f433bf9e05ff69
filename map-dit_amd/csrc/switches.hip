// The switch table (switches.h) and the host-only entry points that belong to neither 16-bit operand format.  No kernel here.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "switches.h"

// ---- error plumbing (shared) ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void mapdit_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* mapdit_last_error(void) { return g_err; }
extern "C" int mapdit_abi_version(void) { return 5; }

// ---- the switches ----------------------------------------------------------------------------------------
static int gemm_phases_arg(int v) { return v == 4 || v == 6 || v == 7 ? v : 2; }

static MapditSwitches from_environment() {
    MapditSwitches s;
    if (const char* v = getenv("MAPDIT_GEMM_TILE")) s.gemm_tile = atoi(v);
    if (const char* v = getenv("MAPDIT_GEMM_PHASES")) s.gemm_phases = gemm_phases_arg(atoi(v));
    if (const char* v = getenv("MAPDIT_GEMM_BAND")) s.gemm_band = atol(v);
    if (const char* v = getenv("MAPDIT_SIDE_JAC")) s.side_jac = v[0] == '1';
    if (const char* v = getenv("MAPDIT_DW_GROUP")) s.dw_group = atoi(v);
    if (const char* v = getenv("MAPDIT_FUSED_RMB")) s.fused_rmb = v[0] - '0';
    if (const char* v = getenv("MAPDIT_ATTN_BWD")) s.attn_bwd = v[0] == '1' ? 1 : v[0] == '2' ? 2 : 0;
    if (const char* v = getenv("MAPDIT_DX16")) s.dx16 = v[0] == '0' ? 0 : v[0] == 'f' ? 2 : 1;
    return s;
}

MapditSwitches& mapdit_switches() {
    static MapditSwitches s = from_environment();
    return s;
}

// Tuning hook of the benchmarking tools (tools/gemm_bench.py) and the tests: overrides what the environment said.
// tile: 0 = by shape | 128 | 256;  phases: 2 | 4 | 6 | 7;  band: 0 = derived from K.  Not for use while launches are in flight elsewhere.
extern "C" void mapdit_gemm_tuning(int tile, int phases, long band) {
    MapditSwitches& s = mapdit_switches();
    s.gemm_tile = tile;
    s.gemm_phases = gemm_phases_arg(phases);
    s.gemm_band = band;
}

// ---- which kernel served the last GEMM call ----------------------------------------------------------------
// Written by the dispatcher (gemm.hip launch(), the group entry point) on the host, per thread; no kernel, no effect on any decision.
mapdit_gemm_plan_t& mapdit_gemm_plan_slot() {
    static thread_local mapdit_gemm_plan_t plan = {};
    return plan;
}
extern "C" int mapdit_gemm_last_plan(mapdit_gemm_plan_t* out) {
    MD_CHECK(out, "gemm_last_plan: null output");
    *out = mapdit_gemm_plan_slot();
    return MAPDIT_OK;
}

// ---- the tile edge of a GEMM launch ----------------------------------------------------------------------
// Output tile edge the dispatcher uses for an [M, N] result.  Exposed so callers can size split-K.
// 256 (8 waves, one workgroup per CU) for results that give most of the chip a tile, 128 (4 waves, two per CU) otherwise:
//  * plain launches: fewer than 128 tiles of 256^2 leave more than half the CUs idle (e.g. [8192, 768] = 96 tiles at a per-GPU
//    batch of 32), while the 128^2 kernel has 4x the tiles for 2x the slots; likewise a launch of little more than one round of the
//    chip (257 ... 320 tiles: the second round runs at most a quarter full - [8192, 2304] = 288 tiles: 46 vs 59 us);
//  * split-K launches fill one round through the K cut either way: there the 128^2 kernel wins for the smallest outputs
//    ([768, 768]: 781 vs 704 TFLOP/s; [3072, 768]: 694 vs 812) and when the cut leaves a workgroup fewer than 24 K-tiles against
//    the 256^2 tile's fixed cost of ~8 K-tiles (fill + fp32 epilogue; [3072, 768] over 8,192 rows: 52 vs 63 us).
// A finer occupancy model (useful tile area x last-round occupancy x a per-flop rate of the 128^2 kernel) fitted the isolated
// launches of tools/gemm_bench.py and LOST in the step at 64 and 128 samples and on DiT-XL/2 (+0.1 ... +0.3 ms): not used.
// K = 0: reduction length not known (the older entry points).
extern "C" int mapdit_gemm_tile_size_k(int M, int N, int K, int split_k_launch) {
    const int force = mapdit_switches().gemm_tile;
    if (force == 128 || force == 256) return force;
    if (!(M >= 512 && N >= 256)) return 128;
    const long t256 = (long)cdiv(M, 256) * cdiv(N, 256);
    if (split_k_launch) {
        if (t256 < 12) return 128;
        // round 4: both edges odd multiples of 128 (DiT-XL's [1152, 1152] weight gradients: 25 tiles of 256^2 for 20.25 tiles of
        // work) - below 85 % useful tile area the 128^2 kernel wins (796 vs 669 TFLOP/s; [4608, 1152] at 90 %: 910 vs 889, left alone)
        if ((double)M * N < 0.85 * (double)t256 * 65536.0) return 128;
        if (K > 0) {
            const long slabs = 256 / t256 > 0 ? 256 / t256 : 1;
            if ((K / 64) / slabs < 24) return 128;
        }
        return 256;
    }
    if (t256 < 128) return 128;
    if (t256 > 256 && t256 <= 320) return 128;
    return 256;
}
extern "C" int mapdit_gemm_tile_size_ex(int M, int N, int split_k_launch) { return mapdit_gemm_tile_size_k(M, N, 0, split_k_launch); }
extern "C" int mapdit_gemm_tile_size(int M, int N) { return mapdit_gemm_tile_size_ex(M, N, 0); }

// ---- how a GEMM launch stages its operand tiles ----------------------------------------------------------
// The scalar-base staging (gemm.hip DmaCtx) keeps every offset of an operand but its 64-bit base in 32 bits - the lane offset, the steps
// between pieces and halves, the advance per K-tile (64 rows of a K-major operand): operands whose extent, rows x ld x 2 bytes, does not
// fit an unsigned 32-bit byte offset stay on the 64-bit lane addresses of stage_half / stage_tile.
extern "C" int mapdit_gemm_dma_extent_ok(long rows, long ld) {
    return rows > 0 && ld > 0 && ld < (1l << 31) && rows < (1l << 32) && (unsigned long)rows * (unsigned long)ld * 2ul < (1ul << 32);
}
// 1 if a launch on tiles of `tile` rows (256: 256 x 256, 128: 128 x 128, 64: 64 x 128) stages that way: every tile inside the result (no
// row or column clamp), no K tail, both operands within the 32-bit extent.  Anything else keeps stage_half / stage_tile.
extern "C" int mapdit_gemm_dma_fast(int layout, int M, int N, int K, int lda, int ldb, int tile) {
    if (layout < MAPDIT_NT || layout > MAPDIT_TN || (tile != 256 && tile != 128 && tile != 64)) return 0;
    const int tn = tile == 256 ? 256 : 128;
    if (M <= 0 || N <= 0 || K <= 0 || M % tile != 0 || N % tn != 0 || K % 64 != 0) return 0;
    const bool a_kmaj = layout == MAPDIT_TN, b_kmaj = layout != MAPDIT_NT;
    return mapdit_gemm_dma_extent_ok(a_kmaj ? K : M, lda) && mapdit_gemm_dma_extent_ok(b_kmaj ? K : N, ldb);
}
