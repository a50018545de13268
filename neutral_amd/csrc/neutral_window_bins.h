/*
 * neutral_window_bins.h -- which bin of a weight window's mesh a cell and an energy fall into: the
 * division by a block's edge and the energy group of the edges.  Shared by the census operations
 * (neutral_comb.hip) and the in-step window of the collision kernels (neutral_history.h:
 * WindowRoulette), so that both name the same bin for the same history.
 */
#ifndef NEUTRAL_AMD_WINDOW_BINS_H
#define NEUTRAL_AMD_WINDOW_BINS_H

#include <hip/hip_runtime.h>

namespace neutral {

/* g(E) = #{i in 0 .. G : e[i] <= E} - 1 where that lies in 0 .. G - 1, else -1 ("outside": below
 * e[0], at or above e[G], NaN).  The edges ascend, so the count is where a bisection of "e[i] <= E"
 * ends: at most seven probes of the 65 entries, comparisons only. */
__device__ __forceinline__ int group_of_edges(const double* e, int ngroups, double energy) {
  int lo = 0, hi = ngroups + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= energy) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo <= ngroups ? lo - 1 : -1; /* (lo == 0 gives -1 too) */
}

/* The division: a checked cell index c lies in 0 .. 2^31 - 1 and the hardware has no integer divide.
 * With l = ceil(log2 d) and m = ceil(2^(31 + l) / d) -- which fits 32 bits, since 2^(l - 1) < d --
 * floor(c / d) = (m * c) >> (31 + l) for every such c (Granlund and Montgomery 1994, theorem 4.2
 * with N = 31: 2^(N + l) <= m * d <= 2^(N + l) + 2^l).  The host computes m and the shift once per
 * call; a lane pays one 32 x 32 -> 64 multiply and a shift.  NEUTRAL_BLOCK_DIVIDE=1 builds the
 * compiler's expansion of a 32-bit unsigned divide instead (profiles/block_window/README.md). */
#ifndef NEUTRAL_BLOCK_DIVIDE
#define NEUTRAL_BLOCK_DIVIDE 0
#endif
struct BlockDivisor {
  unsigned d, m;
  int shift;
  static BlockDivisor of(int block) {
    int l = 0;
    while ((1ull << l) < (unsigned long long)block) {
      ++l;
    }
    const unsigned long long d = (unsigned long long)block;
    return BlockDivisor{(unsigned)block, (unsigned)(((1ull << (31 + l)) + d - 1) / d), 31 + l};
  }
  __device__ int quotient(int c) const {
    if constexpr (NEUTRAL_BLOCK_DIVIDE != 0) {
      return (int)((unsigned)c / d);
    } else {
      return (int)(((unsigned long long)m * (unsigned)c) >> shift);
    }
  }
};

}  // namespace neutral
#endif
