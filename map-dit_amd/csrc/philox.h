// The library's counter-based generator, shared by dataset.hip (the data set's shuffle and posterior noise) and steprng.hip (a
// training step's draws): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written
// from its published definition, and the fp32 normal recipe of mapdit.h, "Device-resident latent data set".  ONE copy: a run is
// reproduced from (seed, step) only while every user draws the same bits from the same words.
//
// Normals are Box-Muller pairs of u = ((w >> 8) + 0.5) 2^-24, w a Philox word: u lies in [2^-25, 1 - 2^-25], so |z| <= sqrt(50 ln 2) =
// 5.89 and the tail beyond it is CUT OFF (4e-9 of the mass per draw).  u has 25 significant bits above 1/2 and is never formed there:
// the upper half is reflected, ln u = log1p(-(1 - u)) and sincospi(2u) = sincospi(2u - 2), and 1 - u has 24 bits again - every argument
// the library functions see is exact, so the result carries their error and nothing else.
//
// No product here feeds an addition, so the results do not depend on -ffp-contract; the files that include this header are built with
// -ffp-contract=fast-honor-pragmas all the same (csrc/Makefile), and box_muller switches contraction off for itself.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;                                              // (the bump after the last round is dead code)
        k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// One Box-Muller pair from two words: (r cos 2 pi u_b, r sin 2 pi u_b), r = sqrt(-2 ln u_a).  kr = the 24-bit draw reflected into the
// lower half where it lies in the upper one; (kr + 0.5) 2^-24 then has at most 24 significant bits.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float* zc, float* zs) {
#pragma clang fp contract(off)
    const uint32_t ka = wa >> 8, kb = wb >> 8;
    const bool ha = ka >> 23, hb = kb >> 23;
    const float va = ((float)(ha ? 0xFFFFFFu - ka : ka) + 0.5f) * 0x1p-24f;      // u_a, or 1 - u_a
    const float vb = ((float)(hb ? 0xFFFFFFu - kb : kb) + 0.5f) * 0x1p-23f;      // 2 u_b, or 2 - 2 u_b
    const float r = sqrtf(-2.0f * (ha ? log1pf(-va) : logf(va)));
    float s, c;
    sincospif(vb, &s, &c);
    *zc = r * c;
    *zs = r * (hb ? -s : s);
}

__device__ __forceinline__ void philox_normal4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, float z[4]) {
    const u32x4 w = philox4x32_10(c0, c1, c2, c3, k0, k1);
    box_muller(w.x, w.y, &z[0], &z[1]);
    box_muller(w.z, w.w, &z[2], &z[3]);
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
