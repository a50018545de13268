/*
 * neutral_inject.h -- one source particle (omp3/neutral.c:575-627), as a device function: what
 * injection puts into every slot (inject_kernel) and what the fixed source puts into a dead one
 * (neutral_comb.hip: launch_source).  One copy of the arithmetic, so that a slot refilled with
 * injection's master key and weight holds injection's particle bit for bit.
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

/* Slot kk of a.p becomes the particle of the stream (pkey = a.pid_base + kk, master_key): position
 * from counter 0, direction from counter 1, at `weight`.  (a.nparticles is not looked at.) */
__device__ __forceinline__ void inject_slot(const InjectArgs& a, const int kk,
                                            const uint64_t master_key, const double weight) {
  const uint64_t pkey = a.pid_base + (uint64_t)kk;

  double rn0, rn1;
  generate_random_numbers(pkey, master_key, 0, rn0, rn1); /* omp3/neutral.c:581 */
  const double px = a.left_off + rn0 * a.width;
  const double py = a.bottom_off + rn1 * a.height;

  const int cellx = a.x_off + find_cell(a.edgex + a.pad, a.local_nx, px);
  const int celly = a.y_off + find_cell(a.edgey + a.pad, a.local_ny, py);

  generate_random_numbers(pkey, master_key, 1, rn0, rn1); /* omp3/neutral.c:611 */
  const double theta = 2.0 * M_PI * rn0;
  double s, c;
  sincos(theta, &s, &c);

  a.p.x[kk] = px;
  a.p.y[kk] = py;
  a.p.cellx[kk] = cellx;
  a.p.celly[kk] = celly;
  a.p.omega_x[kk] = c;
  a.p.omega_y[kk] = s;
  a.p.energy[kk] = a.initial_energy;
  a.p.weight[kk] = weight;
  a.p.dt_to_census[kk] = a.dt;
  a.p.mfp_to_collision[kk] = 0.0;
  a.p.dead[kk] = 0;
}

}  // namespace neutral
#endif
