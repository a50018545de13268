/*
 * neutral_inject.h -- one source particle (omp3/neutral.c:575-627), as a device function: what
 * injection puts into every slot (inject_kernel) and what the fixed source, the described source and
 * the mesh source put into a dead one (neutral_comb.hip: launch_source, launch_described_source,
 * launch_mesh_source).  One copy of the arithmetic, so that a slot refilled with injection's master
 * key, weight and source holds injection's particle bit for bit.
 */
#ifndef NEUTRAL_AMD_INJECT_H
#define NEUTRAL_AMD_INJECT_H

#include "neutral_device.h"
#include "neutral_kernels.h"

namespace neutral {

/* Cell of coordinate c in a monotone edge array: the first ii in [0, n) with
 * edge[ii] <= c < edge[ii+1], or 0 when there is none -- what the linear scan
 * at omp3/neutral.c:590-603 returns, found by bisection. */
__device__ __forceinline__ int find_cell(const double* __restrict__ edge, int n, double c) {
  if (!(c >= edge[0]) || !(c < edge[n])) {
    return 0;
  }
  int lo = 0;
  int hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c < edge[mid]) {
      hi = mid;
    } else {
      lo = mid;
    }
  }
  return lo;
}

/* Where a source particle comes from: a box for counter 0's two samples, an interval of the
 * direction angle for counter 1's first, an interval of energy for its second. */
struct SlotSource {
  double left, bottom, width, height;
  double theta0, theta_width;
  double e_lo, e_hi; /* (e_lo == e_hi: a line, the energy is e_lo exactly) */
};

/* injection's own source (omp3/neutral.c:575-627): a's box, every direction, one energy */
__device__ __forceinline__ SlotSource plain_source(const InjectArgs& a) {
  return SlotSource{a.left_off, a.bottom_off,     a.width,          a.height,
                    0.0,        2.0 * M_PI,       a.initial_energy, a.initial_energy};
}

/* Where a source particle's cell comes from: bisected from its position (injection, the fixed and
 * the described source), or known before the position is drawn (the mesh source: the cell is what
 * was drawn, and a position that rounds onto its upper edge stays in it). */
struct BisectedCell {
  __device__ __forceinline__ void operator()(const InjectArgs& a, double px, double py, int& cellx,
                                             int& celly) const {
    cellx = a.x_off + find_cell(a.edgex + a.pad, a.local_nx, px);
    celly = a.y_off + find_cell(a.edgey + a.pad, a.local_ny, py);
  }
};
struct GivenCell {
  int cellx, celly; /* (global: offsets included) */
  __device__ __forceinline__ void operator()(const InjectArgs&, double, double, int& cx, int& cy) const {
    cx = cellx;
    cy = celly;
  }
};

/* Slot kk of a.p becomes the particle of the stream (pkey = a.pid_base + kk, master_key) out of
 * `from`: position from counter 0, direction and energy from counter 1, at `weight`; its cell from
 * `cell`.  With plain_source(a) the angle is fl(2 pi rn0) and the energy a.initial_energy, as
 * injection has them: 0.0 + fl(w rn0), contracted or not, is fl(w rn0).  (a.nparticles is not
 * looked at.) */
template <class Cell>
__device__ __forceinline__ void inject_slot(const InjectArgs& a, const int kk,
                                            const uint64_t master_key, const double weight,
                                            const SlotSource& from, const Cell& cell) {
  const uint64_t pkey = a.pid_base + (uint64_t)kk;

  double rn0, rn1;
  generate_random_numbers(pkey, master_key, 0, rn0, rn1); /* omp3/neutral.c:581 */
  const double px = from.left + rn0 * from.width;
  const double py = from.bottom + rn1 * from.height;

  int cellx, celly;
  cell(a, px, py, cellx, celly);

  generate_random_numbers(pkey, master_key, 1, rn0, rn1); /* omp3/neutral.c:611 */
  const double theta = from.theta0 + from.theta_width * rn0;
  double s, c;
  sincos(theta, &s, &c);
  const double energy =
      from.e_hi == from.e_lo ? from.e_lo : from.e_lo + rn1 * (from.e_hi - from.e_lo);

  a.p.x[kk] = px;
  a.p.y[kk] = py;
  a.p.cellx[kk] = cellx;
  a.p.celly[kk] = celly;
  a.p.omega_x[kk] = c;
  a.p.omega_y[kk] = s;
  a.p.energy[kk] = energy;
  a.p.weight[kk] = weight;
  a.p.dt_to_census[kk] = a.dt;
  a.p.mfp_to_collision[kk] = 0.0;
  a.p.dead[kk] = 0;
}

/* ... the cell by bisection of the edges */
__device__ __forceinline__ void inject_slot(const InjectArgs& a, const int kk,
                                            const uint64_t master_key, const double weight,
                                            const SlotSource& from) {
  inject_slot(a, kk, master_key, weight, from, BisectedCell{});
}

}  // namespace neutral
#endif
