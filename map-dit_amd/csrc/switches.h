// Every run-time switch of the library, in one table ("Switches").  Filled from the environment ONCE, at first use;
// no other file reads the environment.  switches.hip, which defines it, is compiled once: the bf16 and fp16 builds of the kernel
// files share it, and the host-only entry points that belong to neither format live there too (error string, ABI version, GEMM
// tuning hook, tile-size rule, DMA-staging predicates).
#pragma once

#include "../../include/mapdit.h"

struct MapditSwitches {
    // The three fields mapdit_gemm_tuning sets (it overrides what the environment said):
    // MAPDIT_GEMM_TILE = 128 | 256: force the tile edge of every MFMA launch (0: by shape, mapdit_gemm_tile_size_k)
    int gemm_tile = 0;
    // MAPDIT_GEMM_PHASES: the K loop / kernel of the 256^2 path.  2 = by epilogue (default), 4 = one output quadrant per phase,
    // 6 = the wave-private-epilogue kernel for every epilogue, 7 = the shared-image kernel for every epilogue; anything else is 2
    int gemm_phases = 2;
    // MAPDIT_GEMM_BAND = column tiles per band of the 256^2 kernel's tile order (0: derived from K, gemm.hip launch())
    long gemm_band = 0;
    // MAPDIT_SIDE_JAC = 1: the weight-norm Jacobians run on the engine's side stream beside the next weight-gradient GEMM (measured
    // slower, not the default: engine.hip, mapdit_engine::side).  Decides whether the second slab buffer is carved.
    bool side_jac = false;
    // MAPDIT_DW_GROUP: a block's large weight gradients as one grouped launch.  1 = where the cost model says so (default),
    // 0 = never (a launch each), 2 = whenever feasible (engine.hip dw_group_split)
    int dw_group = 1;
    // MAPDIT_FUSED_RMB: the residual / modulate backward as the dX GEMM's epilogue (engine.hip dx_resid_mod_bwd).  -1 (unset) = for the
    // engines that run the 16-bit gradient stream, 0 = never (dX GEMM + separate pass), 1 = also for fp32 streams up to 32,768 rows,
    // 2 = also for fp32 streams without the row limit
    int fused_rmb = -1;
    // MAPDIT_ATTN_BWD: the fused attention backward at head_dim 64.  0 (unset) = the streaming kernel at 256 tokens, one kernel per head
    // below; 1 = the one-head kernel at 256 tokens too; 2 = the two-pass backward (dq, then dk / dv) at every size
    int attn_bwd = 0;
    // MAPDIT_DX16: the gradient stream between the blocks of a 16-bit engine.  1 (unset) = 16 bits, 0 = fp32 (the 16-bit buffers are
    // not carved), 2 (MAPDIT_DX16=f) = 16 bits in the fp16 engine only
    int dx16 = 1;
};

// The one instance.  Not for writing while launches are in flight elsewhere.
MapditSwitches& mapdit_switches();

// The calling thread's record of what the GEMM dispatcher last decided (mapdit_gemm_last_plan reads it; gemm.hip's launch() and the
// group entry point write it).  One slot for both operand formats.
mapdit_gemm_plan_t& mapdit_gemm_plan_slot();
