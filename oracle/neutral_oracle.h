/*
 * neutral_oracle.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * CPU restatement (plain C + OpenMP) of the over-particle history loop of
 * UoB-HPC/neutral's `omp3` kernel set.  It exists only as the parity checker
 * for the HIP path and as the `cpu_baseline` leg of bench.py.  Nothing under
 * neutral_amd/ may include, link or call it.
 *
 * Every function cites the reference file:line it restates (paths relative
 * to the reference tree).  Data layout is the reference's `-DSoA` Particle
 * (neutral_data.h:45-61) so that oracle and HIP states compare array by array;
 * the arithmetic and its order follow omp3/neutral.c, which is AoS -- layout
 * does not enter any result.
 *
 * Pinning (see DESIGN.md "Oracle"): Threefry2x64-20 is checked bit-for-bit
 * against the reference's own Random123/threefry.h compiled in place
 * (oracle/_ref); the full loop is checked against the three known answers of
 * problems/neutral.tests and against the omp3 event counts / tallies recorded
 * in BASELINE.md section 2.  omp3/neutral.c itself is unbuildable here (it
 * needs the absent parent `arch` project), so no compiled omp3 is used.
 */
#ifndef NEUTRAL_ORACLE_H
#define NEUTRAL_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* neutral_data.h:17-24 */
#define ORC_eV_TO_J 1.60217646e-19
#define ORC_AVOGADROS 6.02214085774e23
#define ORC_BARNS 1.0e-28
#define ORC_PARTICLE_MASS 1.674927471213e-27
#define ORC_MASS_NO 1.0e2
#define ORC_MOLAR_MASS 1.0e-2
#define ORC_MIN_ENERGY_OF_INTEREST 1.0e0
#define ORC_OPEN_BOUND_CORRECTION 1.0e-13

/* neutral_data.h:38-43 */
typedef struct {
  double* keys;
  double* values;
  int nentries;
} OrcCrossSection;

/* neutral_data.h:48-61 (SoA flavour) */
typedef struct {
  double* x;
  double* y;
  double* omega_x;
  double* omega_y;
  double* energy;
  double* weight;
  double* dt_to_census;
  double* mfp_to_collision;
  int* cellx;
  int* celly;
  int* dead;
} OrcParticles;

/* Random123/threefry.h:190-293 with Nrounds = 20 (threefry.h:179) */
void orc_threefry2x64_20(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t k1,
                         uint64_t* out0, uint64_t* out1);

/* omp3/neutral.c:632-652 */
void orc_generate_random_numbers(uint64_t pkey, uint64_t master_key,
                                 uint64_t counter, double* rn0, double* rn1);

/* omp3/neutral.c:498-517; *cs_index receives the bracket index found */
double orc_microscopic_cs_for_energy(const OrcCrossSection* cs, double energy,
                                     int* cs_index);

/* omp3/neutral.c:423-471 */
void orc_calc_distance_to_facet(double x, double y, int pad, int x_off,
                                int y_off, double omega_x, double omega_y,
                                double speed, int particle_cellx,
                                int particle_celly, double* distance_to_facet,
                                int* x_facet, const double* edgex,
                                const double* edgey);

/* omp3/neutral.c:474-495 */
double orc_calculate_energy_deposition(double energy, double weight,
                                       double path_length,
                                       double number_density,
                                       double microscopic_cs_absorb,
                                       double microscopic_cs_total);

/* omp3/neutral.c:560-630.  Fills particles [0, nparticles) whose RNG key is
 * pid_base + index (pid_base = 0 reproduces the reference; a non-zero base is
 * the particle-shard extension of SURVEY section 8(e)).  Arrays are caller
 * allocated. */
void orc_inject_particles(int nparticles, uint64_t pid_base, int local_nx,
                          int local_ny, int pad, double local_particle_left_off,
                          double local_particle_bottom_off,
                          double local_particle_width,
                          double local_particle_height, int x_off, int y_off,
                          double dt, const double* edgex, const double* edgey,
                          double initial_energy, OrcParticles* p);

/* omp3/neutral.c:19-206 (solve_transport_2d -> handle_particles, initial=1).
 * Returns the number of particles processed (the "Particles  N" line);
 * *facets and *collisions are incremented as at omp3/neutral.c:202-203. */
uint64_t orc_solve_transport_2d(int nx, int ny, int global_nx, int global_ny,
                                uint64_t master_key, int pad, int x_off,
                                int y_off, double dt, int ntotal_particles,
                                int nparticles, uint64_t pid_base,
                                OrcParticles* p, const double* density,
                                const double* edgex, const double* edgey,
                                const OrcCrossSection* cs_scatter,
                                const OrcCrossSection* cs_absorb,
                                double* energy_deposition_tally,
                                uint64_t* facets, uint64_t* collisions);

/* Scalar-flux tally (declared, never written, in the reference: neutral_data.h:95):
 * when set (nx*ny doubles), orc_solve_transport_2d also accumulates the path-length
 * estimator sum(weight * segment length) / N per cell, flushed where the energy
 * deposition is.  NULL (default) turns it off.  See neutral_oracle.c. */
void orc_set_scalar_flux_tally(double* tally);

/* ---- the optional tallies and Russian roulette of include/neutral_hip.h ---------
 * Restatements of the definitions that header gives, for the HIP path to be compared
 * with cell by cell and group by group (tests/test_oracle_tallies.py pins them on the
 * CPU first, tests/test_tallies_parity.py compares).  Module-level settings like the
 * flux tally's; everything is off by default and orc_solve_transport_2d then computes
 * the bits it always did.
 *   collision tallies (nx*ny doubles each, both or neither):
 *       collisions[cell] += 1 per collision event,
 *       absorbed[cell]   += weight_before * p_absorb / N per absorption, p_absorb the
 *       value the loop draws against;
 *   current (nx*ny doubles each, both or neither):
 *       jx|jy[cell] += weight * length * omega_x|y / N over the flux tally's segments,
 *       with the weight and direction the segment is flown with;
 *   spectrum (out: 2 * ngroups doubles, ngroups <= ORC_SPECTRUM_MAX_GROUPS; GLOBAL cells
 *   x0 <= cellx < x1, y0 <= celly < y1; out == NULL turns it off):
 *       out[g]           += weight * length / N per segment in the box while
 *                           edges[g] <= E < edges[g+1],
 *       out[ngroups + g] += weight_before * cell_mfp / N per collision in the box whose
 *                           pre-collision energy is in group g;
 *   roulette (w_c, w_s; (0, 0) turns it off): inside an absorption, after the weight has
 *   dropped and after the energy-death rule, a weight below w_c survives with weight w_s
 *   iff rc1 * w_s < weight -- rc1 the second number of the absorption's own draw -- and
 *   dies like an energy death with stored weight 0.0 otherwise.  orc_last_roulette reads
 *   what it did in the most recent orc_solve_transport_2d call. */
#define ORC_SPECTRUM_MAX_GROUPS 64
void orc_set_collision_tallies(double* collisions, double* absorbed);
void orc_set_current_tally(double* jx, double* jy);
void orc_set_spectrum_tally(int ngroups, const double* edges, int x0, int y0,
                            int x1, int y1, double* out);
void orc_set_roulette(double weight_cutoff, double survival_weight);
void orc_last_roulette(uint64_t* killed, uint64_t* survived,
                       double* weight_lost, double* weight_gained);

/* histories of the most recent orc_solve_transport_2d call that ended in a
 * census event (not counted by the reference; needed for particle-steps) */
uint64_t orc_last_census(void);

/* omp3/neutral.c:524-527: serial sum of the tally mesh */
double orc_sum_tally(int nx, int ny, const double* energy_deposition_tally);

/* number of OpenMP threads the loop will use */
int orc_num_threads(void);
void orc_set_num_threads(int n);

#ifdef __cplusplus
}
#endif
#endif
