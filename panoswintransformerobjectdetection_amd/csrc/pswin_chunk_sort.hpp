// One chunk of 64-bit composites sorted in LDS by a whole workgroup, and the composite of a float32 score (gfx950 only).
//
// A composite is (an order-preserving bit pattern of a key) << 32 | (a 32-bit index): unique per candidate, so "the first k, ascending" is
// ONE answer whatever order the work is done in, and equal keys come out in ascending index, as a stable sort leaves them.  A selection is
// a reduction tree of chunk sorts (csrc/pswin_proposals.hip): a workgroup sorts its chunk and keeps the first k, the next pass sorts
// those, until one chunk is left.
#pragma once
#include "pswin_common.hpp"

namespace pswin {

typedef unsigned long long chunk_u64;

constexpr chunk_u64 CHUNK_PAD = ~0ull;      // behind every candidate: its index half is no index

// Bitonic sort of s[0 .. ROWS) in LDS, ascending, by THREADS threads (all of the workgroup; ROWS a power of two >= 2).  The caller has
// filled s and NOT yet synchronised; on return s is sorted and visible to every thread.
template <int ROWS, int THREADS>
__device__ inline void chunk_sort_ascending(chunk_u64* s) {
    static_assert((ROWS & (ROWS - 1)) == 0 && ROWS >= 2, "a bitonic network needs a power of two");
    const int t = threadIdx.x;
    __syncthreads();
    for (int k2 = 2; k2 <= ROWS; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int p = t; p < ROWS / 2; p += THREADS) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
                const chunk_u64 a = s[lo], c = s[hi];
                if ((a > c) == ((lo & k2) == 0)) {
                    s[lo] = c;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
}

// 32 bits that order ASCENDING as the float orders DESCENDING.  +0.0 and -0.0 compare equal as floats, so both map to the pattern of
// +0.0; a NaN lands at one of the two ends (outside every contract here: the order is then unspecified, never an index).
__device__ inline unsigned descending_key(float f) {
    unsigned u = f == 0.f ? 0u : __builtin_bit_cast(unsigned, f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // ascending as the float
    return ~u;
}

__device__ inline chunk_u64 descending_composite(float f, unsigned index) { return ((chunk_u64)descending_key(f) << 32) | (chunk_u64)index; }

}  // namespace pswin
