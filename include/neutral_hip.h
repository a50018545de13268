/*
 * neutral_hip.h -- C ABI of libneutral_hip.so, the MI355X (gfx950) kernel set
 * for UoB-HPC/neutral's over-particle transport path.
 *
 * The library is a drop-in "kernel set" in the reference's sense (reference
 * Makefile:2,83: KERNELS=<dir> selects one implementation of the three
 * functions of neutral_interface.h).  Section 1 declares exactly those three
 * symbols with the reference's signatures; section 2 declares the HBM flavour
 * of the parent project's allocation hooks, through which the unchanged
 * reference loader (neutral_data.c) places its buffers; section 3 holds the
 * extensions that have no reference counterpart (device/stream selection,
 * particle shards for multi-GPU, kernel variant, per-step statistics).
 *
 * Plain C types only: pointers marked [device] are HBM addresses (hipMalloc or
 * any allocator handing out device memory, e.g. a torch CUDA tensor's
 * data_ptr); all other pointers are host addresses.  All entry points are
 * synchronous on return unless stated otherwise.  Fatal errors (HIP failures,
 * allocation failures) print to stderr and exit(EXIT_FAILURE), the behaviour
 * of the reference's TERMINATE sites (omp3/neutral.c:572).
 */
#ifndef NEUTRAL_HIP_H
#define NEUTRAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- data model ------------------------------------------------------------
 * Layout-identical to the reference's types, so a reference translation unit
 * compiled with -DSoA and this library agree on every struct they exchange. */

/* = CrossSection, neutral_data.h:38-43 */
typedef struct {
  double* keys;   /* [device] nentries, strictly increasing, eV */
  double* values; /* [device] nentries, barns */
  int nentries;
} NeutralHipCrossSection;

/* = Particle under -DSoA, neutral_data.h:45-61: a host struct of device arrays */
typedef struct {
  double* x;                /* [device] */
  double* y;                /* [device] */
  double* omega_x;          /* [device] */
  double* omega_y;          /* [device] */
  double* energy;           /* [device] */
  double* weight;           /* [device] */
  double* dt_to_census;     /* [device] */
  double* mfp_to_collision; /* [device] */
  int* cellx;               /* [device] */
  int* celly;               /* [device] */
  int* dead;                /* [device] sticky death flag (omp3/neutral.c:91,245) */
} NeutralHipParticle;

/* ---- 1. the reference kernel interface (neutral_interface.h:11-36) ---------- */

/* Replaces <KERNELS>/neutral.c:solve_transport_2d (omp3/neutral.c:19-40,
 * neutral_interface.h:11-20).  Advances every live local particle by one
 * timestep of length dt: re-samples its distance to collision with the
 * Threefry2x64-20 stream (key = {particle id, master_key}, counter from 0),
 * then processes collision / facet / census events until census or death,
 * adding path-length heating into energy_deposition_tally with f64 atomics.
 *   nx, ny                  local mesh extent without padding
 *   global_nx, global_ny    global mesh extent (reflective outer boundary)
 *   master_key              the timestep number tt (main.c:103)
 *   pad, x_off, y_off       halo depth and rank offsets (0 in the reference)
 *   ntotal_particles        global particle count: tallies are scaled by 1/N
 *   nlocal_particles        [host, in] particles in this store; 0 -> prints
 *                           "Out of particles" and returns
 *   neighbours, edgedx, edgedy, reduce_array0..2   accepted, unused
 *   particles               host struct of [device] arrays from inject_particles
 *   density                 [device] ny*nx, row-major (celly*nx + cellx)
 *   edgex, edgey            [device] nx+1 / ny+1 edge coordinates
 *   cs_*_table              host structs of [device] arrays
 *   energy_deposition_tally [device] ny*nx, accumulated (never zeroed here)
 *   facet_events, collision_events  [host] incremented (omp3/neutral.c:202-203)
 * Prints "Particles  <n processed>" like omp3/neutral.c:205 unless silenced. */
void solve_transport_2d(
    const int nx, const int ny, const int global_nx, const int global_ny,
    const uint64_t master_key, const int pad, const int x_off, const int y_off,
    const double dt, const int ntotal_particles, int* nlocal_particles,
    const int* neighbours, NeutralHipParticle* particles, const double* density,
    const double* edgex, const double* edgey, const double* edgedx,
    const double* edgedy, NeutralHipCrossSection* cs_scatter_table,
    NeutralHipCrossSection* cs_absorb_table, double* energy_deposition_tally,
    uint64_t* reduce_array0, uint64_t* reduce_array1, uint64_t* reduce_array2,
    uint64_t* facet_events, uint64_t* collision_events);

/* Replaces inject_particles (omp3/neutral.c:560-630, neutral_interface.h:23-31).
 * Allocates *particles (host struct + eleven [device] arrays of nparticles
 * elements) and fills particles 0..nparticles-1: position uniform in the
 * source box from stream (id, 0, ctr 0), direction from stream (id, 0, ctr 1),
 * energy = initial_energy, weight 1, dt_to_census = dt, alive.  edgex/edgey are
 * [device].  Returns the number of bytes allocated. */
size_t inject_particles(const int nparticles, const int global_nx,
                        const int local_nx, const int local_ny, const int pad,
                        const double local_particle_left_off,
                        const double local_particle_bottom_off,
                        const double local_particle_width,
                        const double local_particle_height, const int x_off,
                        const int y_off, const double dt, const double* edgex,
                        const double* edgey, const double initial_energy,
                        NeutralHipParticle** particles);

/* Replaces validate (omp3/neutral.c:520-557, neutral_interface.h:35-36): sums
 * the [device] tally in index order on the host, prints
 * "Final global_energy_tally %.15e", looks `params_filename` up in the tests
 * file (default "problems/neutral.tests", neutral_data.h:33) and prints
 * PASSED/FAILED at relative tolerance 1e-3 (neutral_data.h:27). */
void validate(const int nx, const int ny, const char* params_filename,
              const int rank, double* energy_tally);

/* ---- 2. allocation hooks, HBM flavour ---------------------------------------
 * The reference never allocates directly: neutral_data.c:97-105,168-169 and
 * the parent project's mesh/shared-data set-up call these hooks, and the object
 * linked in decides the memory space.  This flavour returns zero-filled HBM
 * (hipMalloc) for the allocate_* family and host memory for allocate_host_*.
 * Each allocate_* returns the bytes allocated. */
size_t allocate_data(double** buf, size_t len);
size_t allocate_float_data(float** buf, size_t len);
size_t allocate_int_data(int** buf, size_t len);
size_t allocate_uint64_data(uint64_t** buf, size_t len);
void allocate_host_data(double** buf, size_t len);
void allocate_host_int_data(int** buf, size_t len);
void deallocate_data(double* buf);
void deallocate_int_data(int* buf);
void deallocate_uint64_data(uint64_t* buf);
void deallocate_host_data(double* buf);
/* send = 1 (RECV): *src [device] -> *dst [host]; send = 0 (SEND): host -> device
 * (neutral_data.c:59-62 reads four edge scalars back with RECV) */
void copy_buffer(const size_t len, double** src, double** dst, int send);
void copy_int_buffer(const size_t len, int** src, int** dst, int send);
/* uploads the host buffer *src into a new [device] buffer *dst, frees *src
 * (neutral_data.c:168-169) */
void move_host_buffer_to_device(const size_t len, double** src, double** dst);

/* ---- 3. extensions (no reference counterpart) -------------------------------- */

enum {
  NEUTRAL_HIP_VARIANT_OVER_PARTICLE = 0, /* one lane owns a history */
  NEUTRAL_HIP_VARIANT_EVENT_SORTED = 1,  /* lanes regrouped by next event */
  NEUTRAL_HIP_VARIANT_TILED = 2          /* tile-sorted streaming with the tally tile in
                                            LDS, then the event-regrouped collision kernel
                                            (default) */
};

typedef struct {
  uint64_t nprocessed;  /* live particles advanced ("Particles  N") */
  uint64_t facets;      /* facet events of the last step */
  uint64_t collisions;  /* collision events of the last step */
  uint64_t census;      /* histories of the last step that ended in a census event */
  double kernel_ms;     /* HIP-event time of the step's kernels on their stream */
  int same_tables;      /* 1 when both cs tables held identical data */
  int variant;          /* kernel variant that ran */
  /* tiled variant only (0 otherwise): HIP-event time of its three stages, the
   * events the streaming kernel handled, and the histories it handed to the
   * collision kernel */
  double sort_ms;
  double stream_ms;
  double collide_ms;
  uint64_t stream_facets;
  uint64_t stream_census;
  uint64_t suspended;
  uint64_t aborted;     /* histories stopped by the event watchdog (2^27 events in one
                           timestep; 0 for every sane input) */
  int stream_passes;    /* streaming passes the step took (1 unless particles outran
                           the LDS tally window and migrated to another tile) */
  uint64_t requeued;    /* tiled variant: times the collision stage put a history back in
                           its wave's ring at the end of a time slice (0 when every
                           wave's share of the collision queue fitted its lanes) */
  uint64_t collide_passes; /* wave-level collision passes of the event-regrouped kernel
                           (variants 1, 2): collisions / (64 * collide_passes) is the
                           lane occupancy of its collision passes */
  int host_syncs;       /* times the call waited for the device (1 for a steady-state
                           step of the tiled variant: the read-back of the counters) */
  int stream_passes_enqueued; /* tiled variant: stream passes enqueued (the last step's
                           count plus one when nothing was waited for in between) */
  int tile_cells;       /* tiled variant: tile edge chosen for the problem (16..128 cells) */
  double export_ms;     /* tiled variant, default mode: HIP-event time of the write-back of
                           the records to the SoA arrays (not part of kernel_ms) */
  int checked_arithmetic; /* 1: the step ran the kernels instantiated with IEEE-checked
                             arithmetic (an input lay outside the fast sequences' proven
                             range: neutral_hip_set_arithmetic below); 0: the fast ones */
  int attempts;          /* times the step's kernels were enqueued (1 in steady state; +1
                            when the device-side check turned the attempt down: a table
                            rewritten in place, input outside the proven range) */
  int host_collectives;  /* several ranks: collectives over the ranks' host links that the
                            step made of its own, beside the exchange itself (which is RCCL on
                            the kernels' stream, or staged through those links as a fallback).
                            0 in steady state: event counters and the flags the ranks act on
                            together travel with the tally, on the device.  A decomposed mesh
                            counts the rounds of its particle exchange here */
  int exchange_ranks;    /* ranks the last tally exchange summed over (1: no exchange) */
  uint64_t steals;       /* tiled variant: times a wave of the collision stage that had emptied
                            its ring took half of what waited in the ring of a wave of its CU */
  uint64_t steals_refused; /* ... waves that would have taken but did not, because the key
                            that tells them who shares their CU (read from the hardware)
                            collected more than twice the waves a CU holds in this launch
                            (workgroups placed late enter themselves on a CU whose first ones
                            have left: that much is expected): the launch then steals nothing
                            (0 on an MI355X) */
  uint64_t stream_hops;  /* tiled variant: histories that left the tally window of the tile they
                            were streaming under with far to go and were handed, INSIDE the stream
                            kernel, to the queue of the tile they had reached (no further pass) */
  uint64_t stream_overflows; /* ... and those that found that tile's queue full and waited for
                            another pass of the stream stage instead (0 unless a tile receives
                            more than its queue holds in one launch) */
  uint64_t stream_batches; /* ... claims of a workgroup on a tile's queue (stream_hops / this =
                            histories a workgroup streams under one window placement) */
  uint64_t stream_idle_polls; /* ... times a workgroup looked for work and found none while
                            histories were still in flight elsewhere */
  uint64_t local_nprocessed; /* several ranks: live particles THIS rank advanced (nprocessed is
                            the sum over the ranks then) */
  double exchange_ms;    /* several ranks: HIP-event time of the step's tally exchange (pack, the
                            two all-reduces, the add into the caller's mesh) on the library's own
                            stream, beside the write-back; 0 with one rank */
  int exchange_rounds;   /* decomposed mesh: rounds of the particle exchange between the ranks'
                            blocks the step took (each: count, pack, exchange, append, more passes) */
  uint64_t emigrants;    /* decomposed mesh: histories THIS rank sent to other ranks' blocks */
  uint64_t weighted_waves; /* tiled variant: waves of the collision stage that were dealt a share of
                            the queue in proportion to what a wave is served (5 : 1 : 1 : 1 over
                            the four waves of a SIMD; 0: equal shares -- a small queue, a partial
                            grid) */
  double stream_clock_ghz;  /* tiled variant: the shader clock the stream kernel and the collision */
  double collide_clock_ghz; /* stage ran at, measured by one wave of every launch over its own life
                               (shader-clock ticks per tick of the constant 100-MHz clock); 0: not
                               measured.  The chip does not hold its nominal 2.4 GHz under every load */
  /* Russian roulette (neutral_hip_set_roulette; 0 when it is off), summed over the ranks: */
  uint64_t roulette_killed;      /* histories it ended */
  uint64_t roulette_survived;    /* histories it kept, with weight w_s */
  double roulette_weight_lost;   /* sum of w over the killed */
  double roulette_weight_gained; /* sum of w_s - w over the survivors */
} NeutralHipStepStats;

/* Number of visible devices (does not initialise a device context). */
int neutral_hip_device_count(void);
/* Selects the device for all following calls of this process. Returns 0 on success. */
int neutral_hip_set_device(int device);
/* Stream for all kernels and copies (a hipStream_t; NULL = the null stream). */
void neutral_hip_set_stream(void* hip_stream);
/* Particle shard: local particle i carries the global id pid_base + i as its
 * RNG key, in inject_particles and solve_transport_2d alike.
 * Default 0 = the reference's numbering. */
void neutral_hip_set_pid_base(uint64_t pid_base);
uint64_t neutral_hip_get_pid_base(void);
/* Kernel variant for solve_transport_2d (NEUTRAL_HIP_VARIANT_*); also read once
 * from the environment variable NEUTRAL_HIP_VARIANT.  Returns 0 on success. */
int neutral_hip_set_variant(int variant);
/* quiet != 0 suppresses the per-step "Particles  N" line. */
void neutral_hip_set_quiet(int quiet);
/* Path of the known-answer file used by validate(). */
void neutral_hip_set_tests_file(const char* path);
/* Statistics of the most recent solve_transport_2d call. */
void neutral_hip_last_step(NeutralHipStepStats* stats);
/* Arithmetic of the event bodies.  Divisions, square roots and the logarithm exist in
 * two instantiations of every history kernel that deliver the same bits wherever both
 * are defined: bare operation sequences, proven exact when every density of the mesh
 * and every key and value of the cross-section tables lies in [2^-100, 2^100], and
 * IEEE-checked ones that accept whatever the reference's C accepts (a true-vacuum cell
 * of density 0 runs on 1/0 = inf there, omp3/neutral.c:127-146,231).
 * NEUTRAL_HIP_ARITH_AUTO (default): decided per step ON THE DEVICE from that step's
 * density mesh and tables -- the fast kernels return at entry when the input is outside
 * the proven range and the step runs checked; nothing to rebuild, nothing to configure.
 * NEUTRAL_HIP_ARITH_CHECKED: always the checked kernels (also: environment variable
 * NEUTRAL_HIP_ARITH=checked).  Returns 0 on success. */
#define NEUTRAL_HIP_ARITH_AUTO 0
#define NEUTRAL_HIP_ARITH_CHECKED 1
int neutral_hip_set_arithmetic(int mode);
/* Resets particles 0..nparticles-1 of an existing store to their injected state
 * (same arguments as inject_particles, no allocation). */
void neutral_hip_reinject_particles(const int nparticles, const int local_nx,
                                    const int local_ny, const int pad,
                                    const double local_particle_left_off,
                                    const double local_particle_bottom_off,
                                    const double local_particle_width,
                                    const double local_particle_height,
                                    const int x_off, const int y_off,
                                    const double dt, const double* edgex,
                                    const double* edgey,
                                    const double initial_energy,
                                    NeutralHipParticle* particles);
/* Particle state and the tiled variant.  The tiled variant works on a private
 * array of records sorted by mesh tile that MIRRORS the SoA store of `particles`.
 * By default solve_transport_2d ends with a pass that writes the records back to the
 * SoA arrays (a permutation of 76 B per particle: 11 ms at 1e8 particles), so the
 * arrays are current whenever it returns, as the reference's are.  In the other
 * direction the arrays are read when the store is first stepped and after anything
 * the library can see rewriting them: inject/reinject, and writes through its own
 * hooks (copy_buffer, copy_int_buffer, neutral_hip_memcpy_h2d, neutral_hip_memset)
 * that land inside the store.  A caller that changes particle arrays BEHIND the
 * library's back (its own kernels, hipMemcpy) must say so with
 * neutral_hip_invalidate_particles() before the next solve_transport_2d; the next
 * step then re-imports the arrays (one pass over the store).
 * lazy != 0 drops that pass: the arrays are written back only by
 * neutral_hip_sync_particles() (or a call that needs them: another variant, reinject,
 * a read through the hooks, free): use it when nothing reads the arrays between
 * timesteps, as main.c with visit_dump = 0 (main.c:91-94,149-152).
 * Memory: the tally, density, edge and table arrays handed to solve_transport_2d must
 * be ordinary (coarse-grained) device memory, e.g. from hipMalloc or the hooks above:
 * the tally is accumulated with hardware f64 atomics (-munsafe-fp-atomics), which do
 * nothing on fine-grained or host-mapped memory. */
void neutral_hip_set_lazy_export(int lazy);
/* Tiled variant: on != 0 lets a history that leaves the tally window it streams under change
 * tiles INSIDE the stream kernel (a queue per tile, claimed by whichever workgroup is free:
 * "asynchronous tile queue") instead of waiting for another sort-and-stream pass.  Same
 * particle bits either way.  Off by default: measured level with the passes on the dense decks
 * and slower on the sparse ones.  Also: NEUTRAL_STREAM_QUEUES=1. */
void neutral_hip_set_stream_queues(int on);
void neutral_hip_sync_particles(NeutralHipParticle* particles);
void neutral_hip_invalidate_particles(NeutralHipParticle* particles);
/* ---- scalar-flux tally -------------------------------------------------------------
 * The reference declares `double* scalar_flux_tally` in NeutralData (neutral_data.h:95)
 * and never allocates or writes it, in any backend; the interface has no argument
 * for it.  This library keeps it when asked: the path-length estimator
 *     flux[cell] += (1 / ntotal_particles) * sum of weight * segment length
 * over the track segments a particle lays down in the cell (what collision, facet
 * and census events move it by; `weight` the weight it travels with), flushed to the
 * mesh exactly where the energy deposition is (facet, census, death).  Same layout
 * and normalisation as energy_deposition_tally: ny*nx doubles, accumulated, never
 * zeroed here, [device] coarse-grained memory.  NULL (default) turns it off, and
 * the kernels that run then are the ones without any flux code.  With it, the
 * tiled variant keeps two 88 x 88-cell windows in LDS instead of one of 128 x 128.
 * With several ranks it is all-reduced per step like the energy tally.
 * Checked against the CPU oracle's restatement of this definition and by what the
 * definition implies (tests/test_scalar_flux.py): in a collision-free deck
 * energy tally / flux is one constant, and the flux sums to speed * dt. */
void neutral_hip_set_scalar_flux_tally(double* device_tally);

/* ---- collision tallies --------------------------------------------------------------
 * Two collision-estimator meshes, scored by the kernels that collide histories:
 *     collisions[cell] += 1 for every collision event in the cell (unnormalised: a count
 *                         held in a double, exact below 2^53)
 *     absorbed[cell]   += (1 / ntotal_particles) * weight_before * p_absorb for every
 *                         absorption in the cell (omp3/neutral.c:231-241: the particle keeps
 *                         weight * (1 - p_absorb); p_absorb = Sigma_a / (Sigma_s + Sigma_a),
 *                         the value the kernel draws against)
 * Same layout and normalisation as energy_deposition_tally: ny*nx doubles, accumulated,
 * never zeroed here, [device] coarse-grained memory.  A history keeps both scores in
 * registers while it collides in one cell and adds them to the meshes once when it leaves
 * it (facet, census, death, end of its time, hand-back by the collision stage), so a run of
 * collisions costs one atomic pair, not one per collision.  The per-cell counts sum exactly
 * to NeutralHipStepStats.collisions of the steps run with them.  With several ranks sharing
 * the mesh both are all-reduced per step like the energy tally; a decomposed mesh tallies
 * each rank's own cells.  Both NULL (default) turns them off, and the kernels that run then
 * are the ones without any of this code.  Returns 0, or 1 -- and changes nothing -- when
 * exactly one of the two is NULL.
 * Checked against the CPU oracle's restatement of this definition, cell by cell (the counts
 * exactly; tests/test_tallies_parity.py), and by what the definition implies
 * (tests/test_collision_tallies.py). */
int neutral_hip_set_collision_tallies(double* collisions, double* absorbed);

/* ---- net current per cell -------------------------------------------------------------
 * The direction of the transport beside its amount: the vector J = (Jx, Jy) per cell,
 *     jx[cell] += (1 / ntotal_particles) * sum of weight * segment length * omega_x
 *     jy[cell] += (1 / ntotal_particles) * sum of weight * segment length * omega_y
 * over exactly the segments of the scalar-flux tally (neutral_hip_set_scalar_flux_tally: a
 * segment ends at a collision, a facet or the census and is scored in the cell it lies in),
 * with the weight and the direction cosines the segment is FLOWN with: before the collision
 * that ends it changes them, and before a reflection at the mesh's edge flips a sign.  With
 * phi the scalar flux of the same steps, |J| <= phi in every cell (0: isotropic, phi: a beam),
 * and a history's segments sum to weight * displacement, whatever it scatters.
 * Same layout, memory kind and life cycle as the other meshes: ny*nx doubles each, [device]
 * coarse-grained memory, accumulated over steps, never zeroed here.  A history keeps the two
 * sums in registers beside its pending flux and adds them to the meshes where the flux is
 * added (facet, census, death, hand-back by the collision stage): two atomics more per flush,
 * two fused multiply-adds per collision.  Every variant scores it; the kernels run the scalar
 * flux's code whether or not a flux tally is set (without one it scores into a mesh of the
 * library's that nobody reads).  Works together with the collision tallies, the spectrum,
 * roulette, lazy export and both arithmetic policies.  With several ranks sharing the mesh both
 * are all-reduced per step on the device like the flux; a decomposed mesh tallies each rank's
 * own cells.  Both NULL (default) turns it off, and the kernels that run then are the ones
 * without any of this code.  Returns 0, or 1 -- and changes nothing -- when exactly one of the
 * two is NULL.  (The ABI version is unchanged: look the symbol up.)
 * Checked against the CPU oracle's restatement of this definition, cell by cell and on decks
 * that collide (tests/test_tallies_parity.py), against a numpy march of collision-free flights
 * and by what the definition implies (tests/test_current.py). */
int neutral_hip_set_current_tally(double* jx, double* jy);

/* ---- outflow per cell and side --------------------------------------------------------
 * The weight that crosses a surface, where every other tally is a volume estimator: for every
 * facet event (omp3/neutral.c:303-380)
 *     out[s * nx*ny + celly*nx + cellx] += weight / ntotal_particles
 * with the cell the history holds as it reaches the facet, the weight it is flown with, and the
 * side s of the facet reached, taken from the direction BEFORE any reflection:
 *     s = 0   -x (west)    an x facet,  omega_x < 0
 *     s = 1   +x (east)    an x facet,  omega_x > 0
 *     s = 2   -y (south)   a y facet,   omega_y < 0
 *     s = 3   +y (north)   a y facet,   omega_y > 0
 * A facet event on the mesh's outer boundary reflects (:333-369) and is scored into that
 * boundary side of its cell as well: that entry is the weight that struck the wall and came
 * back, not a loss.  Inflow into a cell through a side is the neighbour's outflow through the
 * shared side, so in every cell
 *     weight before - weight after - absorbed - died = outflow - inflow    (interior sides),
 * and the entries of a step sum to NeutralHipStepStats.facets / N where every weight is 1.
 * A facet event whose moving axis has a direction cosine of exactly zero neither steps nor
 * reflects in the reference and scores nothing (no finite distance leads to one).
 * device_out: four meshes of ny*nx doubles, row-major, back to back -- 4 * nx * ny doubles,
 * [device] coarse-grained memory, accumulated over steps, never zeroed here; local cells (minus
 * x_off / y_off) like every mesh.  Nothing is pending per history (every facet changes the cell
 * or turns the history round), so suspension, requeue, migration, emigration and a roulette
 * death owe the tally nothing.  Every variant scores it, with one global atomic add per facet
 * (dear where very many histories share few cells: DESIGN.md section 4 item 31); the
 * kernels run the scalar flux's code whether or not a flux tally is set (without one it scores
 * into a mesh of the library's that nobody reads).  Works with both arithmetic policies, lazy
 * export, stream queues, and every other option in any combination.  With several ranks sharing
 * the mesh the step's four meshes are all-reduced on the device like the flux (no host
 * collective); on a decomposed mesh each rank scores the cells it owns, and a history that
 * crosses into another rank's block is scored once, by the rank it leaves -- its arrival scores
 * nothing.  NULL (default) turns it off, and the kernels that run then are the ones without any
 * of this code.  (The ABI version is unchanged: look the symbol up.)
 * Checked per cell and side against a Python replay of the reference's event loop, and by the
 * conservation identities above on the device (tests/test_outflow.py). */
void neutral_hip_set_outflow_tally(double* device_out);   /* 4 * nx * ny doubles, [device]; NULL (default): off */

/* ---- vacuum sides: histories escape through chosen outer sides -------------------------
 * `sides` is a mask over the outflow tally's side numbers: 1 << 0 west, 1 << 1 east, 1 << 2 south,
 * 1 << 3 north.  0 (the default) is the reference: every outer wall reflects.  A facet event at
 * which the reference would reflect (omp3/neutral.c:333-369) through a side whose bit is set does
 * everything a facet event does up to and including the position update -- the two quotients
 * come off mfp_to_collision and dt_to_census, energy deposition, flux, current, spectrum, the
 * outflow (with the weight flown with) and the collision scores are tallied, x and y move onto the
 * wall with the direction the history came with -- and then the history ESCAPES instead of
 * turning: dead = 1 and its time ends (dt_to_census = 0: no census event, no census count; the
 * facet is counted).  Direction, energy, weight, cellx and celly stay as they are: the slot holds
 * the leaked weight where it left.  The two clock fields of a dead slot mean nothing.  A direction
 * cosine of exactly zero on the moving axis neither steps nor reflects, and does not escape.  The
 * wall is the GLOBAL mesh's: on a decomposed mesh the rank that owns the boundary cell applies
 * the rule.  Escaped slots are dead slots to the comb, the sources, the window and the census.
 * The per-facet leakage is the outflow tally's entries on the vacuum sides (N times their sum over
 * a side is the weight NeutralHipEscapeStats reports for it).  The rule lives in the kernels that
 * score the outflow: with sides != 0 they run whether or not an outflow tally is set (without one
 * the step's buffer is scored and added to nothing), and with sides == 0 they compute what they did
 * before, bit for bit.  The default kernels carry none of it.  Process-global like the other step
 * options, read at every solve_transport_2d, may change between steps.  The tiled variant takes
 * stores of fewer than 2^30 particles while a side is vacuum.
 * Returns 0, or 1 -- and changes nothing -- when a bit above 8 is set.  (The ABI version is
 * unchanged: look the symbols up.) */
int neutral_hip_set_vacuum_sides(unsigned sides);
unsigned neutral_hip_get_vacuum_sides(void);
/* the last step's escapes by side and the sum of their raw weights (the units of
 * roulette_weight_lost), summed over the ranks; all zero when no side is vacuum */
typedef struct {
  uint64_t escaped[4];
  double weight[4];
} NeutralHipEscapeStats;
void neutral_hip_last_escape(NeutralHipEscapeStats* out);

/* ---- periodic axes: histories wrap through paired outer sides ----------------------------
 * `axes` is a mask: bit 0 -- x, the west and the east wall are one seam; bit 1 -- y, south and
 * north.  0 (the default) is the reference.  A facet event at which the reference would reflect
 * (omp3/neutral.c:333-369) through side s of a periodic axis does everything a facet event does up
 * to and including the position update, with the direction the history came with -- the two
 * quotients come off mfp_to_collision and dt_to_census; energy deposition, flux, current, spectrum
 * and collision scores are flushed; the outflow tally scores side s of the cell it leaves -- and
 * then, instead of turning, the history WRAPS: its position moves by ONE IEEE addition of a number
 * worked out once per step from the edge arrays, never contracted with the move before it,
 *     west: x + W     east: x - W     south: y + H     north: y - H
 *     W = fl(edgex[global_nx] - edgex[0]),  H = fl(edgey[global_ny] - edgey[0])
 * (the bits of the bank source's periodic shift), and its cell on the moving axis becomes the
 * opposite outermost one: global_nx - 1, 0, global_ny - 1 or 0.  There is no snap: a west or south
 * wrap lands 1e-13 inside the last cell, as any interior crossing toward lower indices does; an
 * east or north wrap lands within rounding of the first edge, as any interior crossing upward.
 * Direction, energy, weight, both clocks and the RNG counter are untouched, and the history goes
 * on in the SAME step in the density of the cell it entered, looked up as at any crossing (the
 * macroscopic cross sections are refreshed where it differs).  The event is one facet in
 * NeutralHipStepStats; it is not a reflection and not an escape: the leakage tally and the escape
 * bank see nothing of it.  A direction cosine of exactly zero on the moving axis neither steps,
 * turns nor wraps.
 * The wall is the GLOBAL mesh's: on a decomposed mesh the rank that owns the boundary cell applies
 * the rule, and a history whose new cell another rank owns stops there and emigrates like any
 * history that crosses into another block (its record carries the shifted position).  Particle
 * shards need nothing.
 * The rule lives where the vacuum rule lives, in the kernels that score the outflow: with an axis
 * set they run whether or not an outflow tally is set, and with axes == 0 they compute what they
 * did before, bit for bit.  The default kernels carry none of it.  Process-global like the other
 * step options, read at every solve_transport_2d, may change between steps.
 * A side is never both: the setter returns 1 -- and changes nothing -- when a bit above 2 is set or
 * a side of a requested axis is currently vacuum, and neutral_hip_set_vacuum_sides refuses a side
 * of a currently periodic axis in the same way.  Otherwise 0.  (The ABI version is unchanged: look
 * the symbols up.) */
int neutral_hip_set_periodic_axes(unsigned axes);
unsigned neutral_hip_get_periodic_axes(void);
/* the last step's wraps by the side LEFT through (the outflow's numbering) and the sum of their
 * raw weights, counted per wave and side as the escapes are and summed over the ranks with the
 * step's other words; all zero when no axis is periodic */
typedef struct {
  uint64_t wrapped[4];
  double weight[4];
} NeutralHipWrapStats;
void neutral_hip_last_wraps(NeutralHipWrapStats* out);

/* ---- leakage tally: the escapes by side, energy group and exit cosine -------------------
 * The partial current through the vacuum sides, scored on the device at the instant a history
 * escapes (neutral_hip_set_vacuum_sides: the facet event at which it would have reflected through a
 * side whose bit is set), in every kernel variant, from the side s the vacuum rule itself uses (the
 * outflow's numbering, 0 west .. 3 north) and the energy E, the weight w and the direction the
 * history arrives with -- the slot keeps all three.
 *   group   G = ngroups, 0 .. 64.  G == 0 takes edges == NULL; G >= 1 takes G + 1 finite, positive,
 *           strictly ascending edges, and the group is found as the census and the in-step window
 *           find it: comparisons only, an energy on an edge belongs to the group above.  g is that
 *           group, or G where there is none (below edges[0], at or above edges[G], NaN); with
 *           G == 0 every escape is in row 0.  Row G, "no group", is kept so that the rows always
 *           close on the escape statistics.
 *   cosine  mu = |omega_x| for sides 0 and 1, |omega_y| for sides 2 and 3: the cosine between the
 *           direction and the outward normal, never 0 (a zero cosine on the moving axis does not
 *           escape).  M = ncosines, 1 .. 64; m = min(M - 1, (int)fl(mu * (double)M)): one IEEE
 *           multiply, a truncation, a clamp -- mu == 1.0 lands in bin M - 1.
 *   bin     b = (s * (G + 1) + g) * M + m
 *     device_out[b]                     += w / ntotal_particles    (the outflow's normalisation)
 *     device_out[4 * (G + 1) * M + b]   += 1.0                     (a count held in a double: exact)
 * device_out: 2 * 4 * (G + 1) * M doubles, [device] coarse-grained memory, accumulated over steps
 * and never zeroed here: a caller that wants the leakage per time interval reads or zeroes it
 * between steps.  The setting persists across steps and the edges are copied at the call.
 * device_out == NULL (the default) turns it off whatever the other arguments are, and touches no
 * device.  Nothing is scored while no side is vacuum, and the kernels that run then are the ones
 * that run today.  What follows: per step and side the counts over all rows and cosines sum to
 * NeutralHipEscapeStats.escaped[s] exactly, and N times the weights to .weight[s] within the
 * summation's rounding; a tally with (G, M) summed over its rows is the tally with (0, M); one
 * with (0, 1) holds the escape statistics and nothing else.
 * With several ranks sharing the mesh the step's bins are all-reduced on the device (no host
 * collective) and every rank's device_out receives the sum; on a decomposed mesh the rank that
 * owns the boundary cell scores, and the sum over the ranks' arrays is the tally.
 * The kernels aggregate per wave and distinct bin (two atomics per wave and bin at most, summed in
 * lane order), not per history.  Returns 0, or 1 -- and changes nothing, decided before any device
 * call -- when ngroups is outside 0 .. 64, edges is NULL with ngroups > 0 or not NULL with
 * ngroups == 0, an edge is not finite, not positive or not above the one before, or ncosines is
 * outside 1 .. 64.  (The ABI version stays 12: detect it by the symbol.)
 * Checked bin by bin against the Python replay of the event loop (tests/leakage_reference.py,
 * tests/test_leakage.py). */
int neutral_hip_set_leakage_tally(int ngroups, const double* edges /* [host] ngroups + 1, or NULL */,
                                  int ncosines, double* device_out /* [device] 2 * 4 * (ngroups + 1) * ncosines */);

/* ---- escape bank: the histories that leave, as a list on the device -----------------------
 * The leakage tally bins what escapes; the bank keeps the escaping histories themselves, so that a
 * second calculation can start from them (neutral_hip_source_bank below): a surface source written
 * at the vacuum sides.  A dead slot keeps the state a history left with, but not the side or the
 * time, and the comb, the sources and the window overwrite it between steps.
 * Every escape of a step (neutral_hip_set_vacuum_sides) claims one index from a cursor the library
 * owns on the device (u64: it never wraps).  An escape whose index is below `capacity` writes its
 * record there; one with a higher index writes nothing and is only counted.  The records of step k
 * occupy [claimed before, claimed after) clipped to capacity; the order inside a step's range is
 * unspecified -- waves race -- and the SET of records is deterministic.  A history escapes at most
 * once per step, so `slot` is unique inside a step's range.
 *   x, y              on the wall, as the slot keeps them (west and south: 1e-13 beyond it -- the
 *                     open bound's correction is part of the distance flown)
 *   omega_x, omega_y  the direction it arrived with
 *   energy, weight    as the slot keeps them
 *   time_left         dt_to_census after the facet event's decrement, before the escape zeroes it:
 *                     the time of flight inside the step is dt - time_left.  (A step resets every
 *                     live history's clock to dt when it begins -- the reference's behaviour --, so
 *                     this is data, not a clock the next problem could go on with.)
 *   slot              the index in this rank's store (no flag bits)
 *   side              0 west .. 3 north, the vacuum rule's own
 * device_records: [device] `capacity` records, 16-byte aligned.  NULL (the default) turns the bank off
 * whatever capacity is, and touches no device.  Otherwise the call returns 1 and changes nothing --
 * decided before any device call -- when capacity == 0 or the pointer is not 16-byte aligned.  A
 * successful call sets `claimed` to 0.  The setting is process-global and persists across steps.
 * neutral_hip_reset_escape_bank sets the cursor to 0 and leaves the records as they are (returns 0;
 * 1 while the bank is off).
 * Stats: claimed is the cursor, recorded = min(claimed, capacity), step_* the last step's
 * increments.  On one rank step_claimed equals the sum of NeutralHipEscapeStats.escaped[] of that
 * step, exactly.
 * Nothing is recorded while no side is vacuum, and the kernels that run then are the ones that run
 * without the bank; with sides set it rides the instantiations that score the outflow, like the
 * vacuum mask and the leakage tally, in every kernel variant.  The kernels aggregate per wave: one
 * returning atomic on the cursor per wave and trip of the facet loop in which a lane escapes, never
 * one per history, and four 16-byte stores per record.  The host reads the cursor with the step's
 * other results: a step with the bank off gets no additional synchronisation or copy.
 * With several ranks sharing a mesh each rank has its own bank, its own cursor and its own stats;
 * there is no collective, `slot` indexes the rank's shard, and over the ranks the step_claimed
 * values sum to the escape statistics.  On a DECOMPOSED store the step runs as without the bank and
 * records nothing (step_claimed == 0).
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked record by record against the Python replay of the event loop
 * (tests/escape_bank_reference.py, tests/test_escape_bank.py). */
typedef struct {                 /* 64 bytes, 16-byte aligned */
  double x, y;
  double omega_x, omega_y;
  double energy, weight;
  double time_left;
  uint32_t slot;
  uint32_t side;
} NeutralHipEscapeRecord;

int neutral_hip_set_escape_bank(NeutralHipEscapeRecord* device_records, uint64_t capacity);
int neutral_hip_reset_escape_bank(void);
typedef struct {
  uint64_t capacity, claimed, recorded, step_claimed, step_recorded;
} NeutralHipEscapeBankStats;
void neutral_hip_escape_bank_stats(NeutralHipEscapeBankStats* out);

/* ---- energy-group flux spectrum over a box of cells ---------------------------------
 * Group g is edges[g] <= E < edges[g+1] (g = 0 .. ngroups-1), E the energy a history travels
 * with; energies outside [edges[0], edges[ngroups]) are not scored.  The box is the GLOBAL
 * cells x0 <= cellx < x1, y0 <= celly < y1; (0, 0, global_nx, global_ny) is the whole mesh.
 *     device_out[g]           += (1/N) * sum of weight * segment length over the segments laid
 *                                down inside the box while the energy is in group g: the
 *                                segments, weights and 1/N (ntotal_particles) of the scalar-flux
 *                                tally, a segment running between two events (collision, facet,
 *                                census) and scored in the cell it lies in
 *     device_out[ngroups + g] += (1/N) * sum of weight_before / Sigma_t(E_before) over the
 *                                collisions inside the box whose pre-collision energy is in
 *                                group g, Sigma_t = 1 / cell_mfp the macroscopic total cross
 *                                section the collision distance was sampled with
 * The distance to a collision is drawn as in the reference (omp3/neutral.c: -log(rn) / Sigma_s of
 * the cell where it is drawn, in mean free paths of the cell it is flown in), so the two
 * estimators share their expected value where Sigma_s is 1/m in every cell a flight crosses;
 * elsewhere the collision value follows this sampling, not the flux.  It is noisy in near-vacuum
 * cells and a true vacuum (density 0) never collides: there the track-length value is the one
 * to use.  device_out: 2 * ngroups doubles, [device]
 * coarse-grained memory, accumulated over steps and never zeroed here.  With several ranks
 * sharing the mesh the step's values are all-reduced on the device and every rank's device_out
 * receives the sum; a decomposed mesh scores each rank's own cells of the box (the sum over
 * the ranks is the spectrum).  device_out == NULL (the default) turns it off, whatever the
 * other arguments, and the kernels that run then are the ones without any of this code.  The
 * setting persists across steps.  Returns 0, or 1 -- and changes nothing -- when ngroups is
 * outside 1..64, an edge is not finite or not positive, the edges are not strictly
 * ascending, or the box is empty or has a negative origin.  (The library does not know the
 * mesh when this is called: a box that reaches beyond it covers the cells of it it contains.
 * The ABI version stays 12: detect it by the symbol.)
 * Checked against the CPU oracle's restatement of this definition, both estimators group by
 * group, an edge exactly at the source's energy included (tests/test_tallies_parity.py), and
 * by what the definition implies (tests/test_spectrum.py). */
int neutral_hip_set_spectrum_tally(int ngroups, const double* edges, int x0, int y0, int x1, int y1,
                                   double* device_out);

/* ---- weight cutoff with Russian roulette --------------------------------------------
 * The reference's implicit capture (omp3/neutral.c:231-241) never ends a history for low
 * weight: an absorption multiplies it by 1 - p_absorb, and only an energy below
 * MIN_ENERGY_OF_INTEREST ends it.  With a weight cutoff w_c > 0 and a survival weight
 * w_s >= w_c set, an absorption plays Russian roulette:
 *   - only inside an absorption, after the weight has dropped to
 *     w = weight * (1 - p_absorb) -- the only place the weight changes;
 *   - the energy-death rule comes first: an absorbed history below 1 eV dies as without
 *     roulette, and plays none;
 *   - when w < w_c, the sample is the SECOND number of the absorption's draw, rn1[1] =
 *     u64_to_unit(r1) (omp3/neutral.c:646-651), which a scatter takes for its cosine and an
 *     absorption leaves unused: the RNG counter schedule does not change;
 *   - the history survives iff fl(rn1[1] * w_s) < w (one IEEE f64 multiply, the same in both
 *     arithmetic policies) and goes on with weight w_s; otherwise it dies there, exactly like
 *     an energy death: dead = 1, its pending energy deposition, flux and collision scores go
 *     to its cell, and its stored weight becomes 0.0.
 * Nothing else depends on the weight -- positions, directions, energies, dt_to_census,
 * mfp_to_collision, cells, the RNG counter -- so a history's path with roulette on is bit for
 * bit its path with roulette off, up to where roulette kills it.  The game is fair: survival
 * has probability w / w_s, so the expected weight, hence every tally, is unchanged.  The
 * collision tallies score weight_before * p_absorb, taken before roulette.
 * NeutralHipStepStats.roulette_* report what it did per step (summed over the ranks).
 * Roulette is a compile-time property of the kernels that collide: (0, 0), the default,
 * turns it off, and the kernels that run then are the ones without any of this code.  The
 * setting persists across steps.  Returns 0, or 1 -- and changes nothing -- when either value
 * is NaN, infinite or negative, when exactly one of them is 0, or when
 * survival_weight < weight_cutoff, or -- for a non-zero pair -- while an in-step weight window is
 * set (neutral_hip_set_window_roulette: the two are exclusive).  (The ABI version stays 12: detect
 * it by the symbol.)
 * Checked against the CPU oracle's restatement of this definition, history by history (who
 * was killed, who survived, exactly; tests/test_tallies_parity.py), and by what the
 * definition implies (tests/test_roulette.py). */
int neutral_hip_set_roulette(double weight_cutoff, double survival_weight);

/* ---- census weight comb: population control between timesteps -----------------------
 * The store has a fixed size: a history that ends (energy below 1 eV, or killed by roulette)
 * keeps its slot for good, and a roulette survivor goes on at w_s beside neighbours of weight 1.
 * The comb (Booth's weight comb) is roulette's other half: called between two
 * solve_transport_2d calls -- nothing is pending then, every score is flushed at census -- it
 * resamples the census population to n equal weights, refills every dead slot and preserves
 * every expected value.  With n = nparticles (for a sharded store created by inject_particles:
 * the shard's count, as neutral_hip_reinject_particles treats it):
 *   live weight   lw_j = weight[j] if dead[j] == 0, otherwise 0
 *   prefix sums   S_j = lw_0 + ... + lw_j (inclusive), S_{-1} = 0, W = S_{n-1}, delta = W / n
 *   offset        v = 1 - rn0, (rn0, .) = generate_random_numbers(pkey = UINT64_MAX - pid_base,
 *                 master_key = seed, counter = 0): the library's Threefry and u64_to_unit; rn0 lies
 *                 in (0, 1], v in [0, 1); no particle carries that key
 *   teeth         tooth k (k = 0 .. n-1) sits at t_k = (k + v) * delta and selects the one live j
 *                 with S_{j-1} <= t_k < S_j: src[k]
 *   new slot k    a copy of particle src[k]: x, y, omega_x, omega_y, energy, dt_to_census,
 *                 mfp_to_collision, cellx and celly bit for bit; weight = delta, the same double in
 *                 every slot; dead = 0
 * src is non-decreasing: copies of one particle are contiguous and the layout is deterministic.
 * A particle's random stream is keyed by its slot, so a copy in another slot is an independent
 * history from the next step on.  The prefix sums are within 64 eps W of the exact sums (a blocked
 * scan, never a running sum over the store); a tooth nearer than that to a boundary S_j may go
 * to either neighbour.  The same input gives the same bits on every call.
 * Returns 0: done.  1: nothing changed -- no particle is live, W is not a positive finite number,
 * or a live weight is negative or not finite (found on the device, in the scan).  2: nothing
 * changed -- the store is decomposed (a comb over the ranks' blocks is not offered).
 * Several ranks sharing the mesh: each rank combs its own shard -- its W, its n, its offset
 * through pid_base; fair per shard, and the 1/N of the tallies is unaffected because weight is
 * conserved.  Works the same for every kernel variant: pending record state of the tiled variant
 * is written back first (lazy export included) and the next step imports the arrays again.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked against a numpy restatement of this definition, tooth for tooth, and inside a run
 * against the CPU oracle (tests/test_comb.py). */
typedef struct {
  uint64_t live_before;    /* particles with dead == 0 going in */
  uint64_t sources_kept;   /* distinct particles that received at least one tooth */
  uint64_t max_copies;     /* most teeth on one particle */
  double weight_before;    /* W: sum of the live weights going in */
  double weight_each;      /* W / n: the weight every slot holds coming out */
  double comb_ms;          /* HIP-event time of the comb's kernels */
} NeutralHipCombStats;

int neutral_hip_comb_particles(NeutralHipParticle* particles, int nparticles,
                               uint64_t seed, NeutralHipCombStats* stats /* may be NULL */);

/* ---- fixed source: dead slots refilled with new particles between timesteps ----------
 * inject_particles fills the store once, and a history that ends keeps its slot for good; the comb
 * refills such slots, but only with copies of what is still alive.  This call adds particles: it
 * finds the dead slots of a store on the device and turns the first `count` of them into fresh
 * source particles -- a source that emits at a steady rate, step after step, until emission
 * balances absorption.
 * Which slots.  Called between two solve_transport_2d calls: nothing is pending then.  With n =
 * nparticles (for a sharded store created by inject_particles: the shard's count, exactly as
 * neutral_hip_comb_particles chooses it), let d_0 < d_1 < ... be the indices j with dead[j] != 0.
 * The slots d_0 .. d_{m-1}, m = min(count, number of dead), are refilled, in ascending index
 * order: deterministic, found by one scan, and filled by lanes whose stores ascend.  No other
 * slot is touched, live or dead, in any field, not even in bits that are NaN.
 * What a refilled slot j holds: exactly what injection (inject_particles) would put there with the
 * master key `seed` in place of 0 and `weight` in place of 1.0 -- position from the stream
 * (pkey = pid_base + j, master_key = seed, counter 0) in the box (left_off, bottom_off, width,
 * height), cell by bisection of the edges, direction from counter 1, energy = initial_energy,
 * dt_to_census = dt, mfp_to_collision = 0, dead = 0.  Injection and the source run one device
 * function, so with seed = 0, weight = 1.0 and the arguments of the store's injection a refilled
 * slot gets back, bit for bit, the particle inject_particles put there.  The arguments from
 * local_nx to initial_energy are those of neutral_hip_reinject_particles, with their meaning.
 * Which seeds are safe: the timestep tt draws from master key tt and injection from master key 0,
 * so a caller passes seeds that no timestep number uses; this project's Python wrapper and driver
 * pass 2^63 + tt.  A slot refilled twice with one seed holds the same particle twice.
 * Units: `weight` is in the tallies' units -- 1 is one of the N particles (ntotal_particles) the
 * tallies are normalised by; the 1/N of the tallies does not change.
 * Returns 0: done -- also when fewer than `count` slots were dead, or none: stats->emitted says how
 * many were refilled.  With emitted == 0 nothing is written and a tiled store is not invalidated:
 * the next step pays no re-import.  1: nothing changed -- particles is NULL, n <= 0, count < 0;
 * weight, initial_energy or dt is not finite and positive; width or height is negative or not
 * finite; an edge array is NULL, local_nx or local_ny is below 1, or pad is negative.  2: nothing
 * changed -- the store is decomposed, as for the comb.
 * Several ranks sharing the mesh: each rank refills its own shard -- its n, its count, its keys
 * through pid_base.  Works the same for every kernel variant: pending record state of the tiled
 * variant is written back first (lazy export included), and after a refill the records are
 * dropped, so that the next step imports the arrays again -- slots of the tiled pipeline's
 * graveyard included.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked slot for slot against injection's own bits and a numpy restatement of this definition,
 * and inside a run against the CPU oracle (tests/test_source.py). */
typedef struct {
  uint64_t dead_before;    /* slots with dead != 0 going in */
  uint64_t emitted;        /* slots refilled: min(count, dead_before) */
  double weight_emitted;   /* emitted * weight */
  double source_ms;        /* HIP-event time of the call's kernels */
} NeutralHipSourceStats;

int neutral_hip_source_particles(NeutralHipParticle* particles, int nparticles, int count,
                                 double weight, uint64_t seed,
                                 /* the arguments of neutral_hip_reinject_particles that describe the source: */
                                 const int local_nx, const int local_ny, const int pad,
                                 const double left_off, const double bottom_off,
                                 const double width, const double height,
                                 const int x_off, const int y_off, const double dt,
                                 const double* edgex, const double* edgey,
                                 const double initial_energy,
                                 NeutralHipSourceStats* stats /* may be NULL */);

/* ---- described source: components with a box, an energy spectrum and a direction interval ----
 * The fixed source above emits from one box, at one energy, in every direction.  This call takes a
 * description instead: up to 16 components, each with a relative emission rate (share), a box, an
 * interval of the direction angle and a spectrum -- a run of the table of energy bins, each bin
 * with a share of its own; a bin with e_lo == e_hi is a line.  Two sources, a beam, a source with a
 * spectrum: all are descriptions.
 * Which slots: exactly as neutral_hip_source_particles -- the first min(count, number of dead) dead
 * slots in ascending index order, n chosen as that call chooses it (the shard's count for a sharded
 * store), and no other slot touched in any field.
 * Cumulative shares, made on the host as running sums in doubles, left to right, one IEEE addition
 * each: C_0 = share_0, C_k = fl(C_{k-1} + share_k), S = C_{K-1} over the components; B_{k,0}, ...
 * and their last, S_k, over component k's bins in order.
 * What a refilled slot j holds.  Its stream is pkey = pid_base + j, master_key = seed; counters 0
 * and 1 are used exactly as injection uses them, counter 2 is this call's:
 *   counter 2, (u0, u1): t = fl(u0 * S); the component k is the first with t < C_k, else K - 1 (the
 *     samples lie in (0, 1], so t == S can happen).  tb = fl(u1 * S_k); the bin b is the first of
 *     k's bins with tb < B_{k,b}, else the last.  Single multiplications and comparisons.
 *   counter 0, (p0, p1): position in k's box by injection's own expression, left + p0 * width and
 *     bottom + p1 * height; cellx, celly by bisection of the edges.
 *   counter 1, (d0, d1): theta = theta0 + theta_width * d0 and omega = (cos theta, sin theta);
 *     energy = e_lo + d1 * (e_hi - e_lo), and e_lo exactly for a line.  (Injection leaves d1 unused.)
 *   weight = weight, dt_to_census = dt, mfp_to_collision = 0, dead = 0.
 * Injection, the fixed source and this call run one device function.  So one component with a
 * store's own box, (0.0, 2.0 * M_PI) and one line at initial_energy gives, bit for bit in all eleven
 * fields, what neutral_hip_source_particles gives with the same count, weight and seed; with seed 0
 * and weight 1 that is what inject_particles put there.  Seeds: as for the fixed source.
 * Returns 0: done; emitted == 0 writes nothing and does not invalidate a tiled store.  1: nothing
 * changed -- a refusal of neutral_hip_source_particles that applies here (particles, n, count,
 * weight, dt, the edges, local_nx, local_ny, pad); ncomponents outside 1..16; nbins outside 1..256; a
 * NULL table; a share, of a component or a bin, that is not finite and > 0, or shares whose running
 * sum is not finite; a width or height that is negative or not finite; left, bottom or theta0 not
 * finite; theta_width negative or not finite; bin_count < 1 or a bin range outside the table; e_lo
 * not finite and > 0, e_hi not finite, or e_hi < e_lo.  2: the store is decomposed.
 * Like the fixed source, the call checks neither that a box lies inside the mesh (a position outside
 * it gets cell 0) nor that the energies lie inside the caller's cross-section tables; this project's
 * Python wrapper does (SourceDescription.check).
 * stats->emitted_by_component[k]: the refilled slots that came out of component k; they sum to
 * emitted.  Several ranks sharing a mesh: each rank refills its own shard with the same description.
 * Every kernel variant, lazy export included: records are written back first and dropped after a
 * call that wrote, as for the fixed source; the next step's import looks up the cross sections for
 * every slot's own energy.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked against the fixed source's bits, a numpy restatement of this definition, the CPU oracle in
 * a run, and a closed form (tests/test_described_source.py). */
typedef struct {
  double share;                        /* relative emission rate, finite, > 0 */
  double left, bottom, width, height;  /* the box, as neutral_hip_source_particles takes one */
  double theta0, theta_width;          /* direction angle uniform over [theta0, theta0 + theta_width];
                                          (0.0, 2.0 * M_PI) is injection's isotropic source */
  int bin_first, bin_count;            /* its energy spectrum: bins[bin_first .. bin_first + bin_count) */
} NeutralHipSourceComponent;

typedef struct { double e_lo, e_hi, share; } NeutralHipSourceBin;  /* e_lo == e_hi: a line */

typedef struct {
  uint64_t dead_before, emitted;
  uint64_t emitted_by_component[16];
  double weight_emitted;               /* emitted * weight */
  double source_ms;
} NeutralHipDescribedSourceStats;

int neutral_hip_source_described(NeutralHipParticle* particles, int nparticles, int count,
                                 double weight, uint64_t seed,
                                 int ncomponents, const NeutralHipSourceComponent* components /* [host] */,
                                 int nbins, const NeutralHipSourceBin* bins /* [host] */,
                                 const int local_nx, const int local_ny, const int pad,
                                 const int x_off, const int y_off, const double dt,
                                 const double* edgex, const double* edgey,
                                 NeutralHipDescribedSourceStats* stats /* may be NULL */);

/* ---- mesh source: emit in proportion to a per-cell strength mesh ---------------------------
 * The two sources above emit from boxes somebody wrote down.  This call emits from a mesh on the
 * device instead -- one of the library's own tallies (what was absorbed, for a regeneration run) or
 * another calculation's result: cell c = j * local_nx + i of this rank's block has strength s_c
 * (strength: local_ny rows of local_nx doubles), and a new particle is born in cell c with
 * probability s_c / S, uniformly inside it.  One energy spectrum (a table of bins as the described
 * source takes it, all of it) and one interval of the direction angle serve every cell.
 * Which slots: exactly as neutral_hip_source_particles -- the first min(count, number of dead) dead
 * slots in ascending index order, n chosen as that call chooses it (the shard's count for a sharded
 * store), and no other slot touched in any field.
 * The cumulative mesh: C_c, the inclusive prefix sum of the strengths in cell order, and S, the last
 * of them, made by the device's f64 scan in its own fixed order: within 64 eps S of the exact sums,
 * and the same input always gives the same bits.  B_b and their last, S_B: the running sums of the
 * bins' shares, made on the host, left to right, one IEEE addition each.
 * What a refilled slot holds.  Its stream is pkey = pid_base + slot, master_key = seed:
 *   counter 2, (u0, u1): t = fl(u0 * S); the cell is the first c with t < C_c; when there is none
 *     (the samples lie in (0, 1], so t == S can happen) the last one with s_c > 0.  A cell with
 *     s_c == 0 is never chosen, whatever the rounding of the scan does at tile and lane seams: the
 *     search runs over the cells with s_c > 0 alone.  tb = fl(u1 * S_B); the bin b is the first with
 *     tb < B_b, else the last -- as the described source chooses a component's bin.
 *   counter 0, (p0, p1): position in the cell's box by injection's own expression, left + p0 * width
 *     and bottom + p1 * height, with left = edgex[pad + i], width = fl(edgex[pad + i + 1] -
 *     edgex[pad + i]) and likewise in y.  cellx = x_off + i and celly = y_off + j are the drawn cell,
 *     written as drawn and not bisected from the position: a position that rounds onto the cell's
 *     upper edge stays in its cell, and the transport treats it as it treats a particle on a facet.
 *   counter 1, (d0, d1): theta = theta0 + theta_width * d0 and omega = (cos theta, sin theta);
 *     energy = e_lo + d1 * (e_hi - e_lo), and e_lo exactly for a line -- as the described source.
 *   weight = weight, dt_to_census = dt, mfp_to_collision = 0, dead = 0.
 * Injection, the other two sources and this call run one device function, which here is handed the
 * cell instead of bisecting for it.  So a mesh whose only non-zero cell is (i, j), with the same bins
 * and angle interval, gives bit for bit in all eleven fields what neutral_hip_source_described gives
 * with one component whose box is that cell (left, bottom, width, height as above) -- but for a
 * position that lands on an edge.  Seeds: as for the fixed source.
 * Returns 0: done; emitted == 0 writes nothing and does not invalidate a tiled store.  1: nothing
 * changed -- a refusal of neutral_hip_source_particles that applies here (particles, n, count,
 * weight, dt, the edges, local_nx, local_ny, pad), or a mesh of more than 2^30 cells; a NULL strength;
 * theta0 not finite, theta_width negative or not finite; nbins outside 1..256, a NULL table, a
 * share that is not finite and > 0 or shares whose sum is not finite, e_lo not finite and > 0, e_hi
 * not finite, or e_hi < e_lo; and, found on the device before anything is written (whether or not a
 * slot is dead): a strength that is negative or not finite, or S not finite and > 0 -- a mesh of
 * zeros.  The stats of such a call say what the device found (dead_before, cells_nonzero,
 * strength_total); emitted is 0.  2: the store is decomposed.
 * Like the other sources, the call does not check that the energies lie inside the caller's
 * cross-section tables; this project's Python wrapper does (MeshSource.check).
 * Several ranks sharing a mesh: each rank refills its own shard from the same mesh.  Every kernel
 * variant, lazy export included: records are written back first and dropped after a call that
 * wrote, as for the fixed source.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked against the described source's bits, a numpy restatement of this definition, the CPU oracle
 * in a run, and a closed form (tests/test_mesh_source.py). */
typedef struct {
  uint64_t dead_before, emitted;
  uint64_t cells_nonzero;   /* K: cells with strength > 0 */
  double strength_total;    /* S as the device summed it */
  double weight_emitted;    /* emitted * weight */
  double source_ms;
} NeutralHipMeshSourceStats;

int neutral_hip_source_mesh(NeutralHipParticle* particles, int nparticles, int count,
                            double weight, uint64_t seed,
                            const double* strength /* [device] local_ny rows of local_nx */,
                            double theta0, double theta_width,
                            int nbins, const NeutralHipSourceBin* bins /* [host] */,
                            const int local_nx, const int local_ny, const int pad,
                            const int x_off, const int y_off, const double dt,
                            const double* edgex, const double* edgey,
                            NeutralHipMeshSourceStats* stats /* may be NULL */);

/* ---- bank source: refill dead slots from a list of escape records ------------------------
 * The fourth source: nothing is sampled and no random number is drawn; the slots are filled from
 * records an escape bank holds (neutral_hip_set_escape_bank above) -- the read side of a surface
 * source.  Coupling is by whole steps: what escapes during step k can enter the next problem before
 * its step k + 1, with a full dt (the step resets the clock anyway).
 * Which slots: the fixed source's.  d_0 < d_1 < ... are the dead slots, m = min(count, number of
 * dead); slot d_k takes record records[first + k].  No other slot is touched in any field.
 * What slot d_k holds, r its record, every operation ONE IEEE f64 operation, not contracted:
 *   x = fl(r.x + shift[2 * r.side]), y = fl(r.y + shift[2 * r.side + 1])    (shift NULL: zeros)
 *   per axis, lo = edge[pad], hi = edge[pad + n]:  0 < lo - p <= snap: p = lo;  0 < p - hi <= snap:
 *     p = hi.  `snapped` counts the coordinates moved.  (An escape on the west or south wall lies
 *     1e-13 beyond it; taken to a mesh with the same origin it lies 1e-13 outside: such a record is
 *     neither refused nor silently bisected to cell 0 -- the caller says how far is near enough.)
 *   the cell per axis: the largest c in [0, n - 1] with edge[pad + c] <= p; where p == edge[pad + c],
 *     that axis' cosine is negative and c > 0, the cell is c - 1: a history on an edge starts in the
 *     cell it moves into, one on the top wall in the last cell.  x_off / y_off are added as
 *     injection adds them.
 *   omega_x, omega_y, energy: the record's.  weight = fl(r.weight * weight_scale).
 *   dt_to_census = dt, mfp_to_collision = 0, dead = 0.
 * Validation runs on the device before anything is written, over the m records that would be used.
 * A record is bad when side > 3; a field is not finite; weight or energy is not positive; both
 * cosines are zero; or a shifted coordinate lies outside [lo, hi] by more than snap.
 * Returns 0: done; emitted == 0 writes nothing and does not invalidate a tiled store.
 *         1: nothing changed -- particles, records or an edge array NULL, n, count, local_nx,
 *            local_ny or pad as the fixed source refuses them, dt or weight_scale not finite and
 *            positive, snap negative or not finite, a shift that is not finite.
 *         2: the store is decomposed.
 *         3: a record is bad; nothing is written, first_bad is the lowest bad index (into records[],
 *            first included), emitted is 0.  Otherwise first_bad is UINT64_MAX.
 * Several ranks sharing a mesh: each rank refills its own shard from the records it is given.
 * Every kernel variant, lazy export included: records of the tiled store are written back first
 * and dropped after a call that wrote, as for the fixed source.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked bit for bit against a numpy restatement of this definition
 * (tests/escape_bank_reference.py, tests/test_escape_bank.py). */
typedef struct {
  uint64_t dead_before, emitted, snapped, first_bad;
  double weight_emitted; /* the sum of the weights written, per wave and then atomically: the order
                            of the waves is not fixed, so it is good to the summation's rounding */
  double source_ms;
} NeutralHipBankSourceStats;

int neutral_hip_source_bank(NeutralHipParticle* particles, int nparticles,
                            const NeutralHipEscapeRecord* records /* [device] */, uint64_t first, int count,
                            double weight_scale,
                            const double* shift /* [host] 8: dx, dy for side 0..3; NULL: zeros */,
                            double snap,
                            const int local_nx, const int local_ny, const int pad,
                            const int x_off, const int y_off, const double dt,
                            const double* edgex, const double* edgey,
                            NeutralHipBankSourceStats* stats /* may be NULL */);

/* ---- census weight window: split and roulette per cell between timesteps --------------
 * Roulette in the collision kernels, the comb and the fixed source are global.  A weight window
 * is population control over the mesh: every cell carries a lower bound for the weight of the
 * histories inside it; heavier histories are split into several lighter ones, lighter ones play
 * Russian roulette, and each cell then holds many histories of about the weight its importance
 * calls for.  Called between two solve_transport_2d calls: nothing is pending then.
 * With n = nparticles (for a sharded store created by inject_particles: the shard's count, exactly
 * as neutral_hip_comb_particles chooses it), for slot j: c = celly[j] * nx + cellx[j] (global cell
 * numbers; lower is the global mesh, ny rows of nx), w_lo = lower[c], w_hi = fl(upper_ratio * w_lo),
 * w_s = fl(survival_ratio * w_lo), w = weight[j].  Every operation below is ONE IEEE f64 operation,
 * in this order, so that a restatement in another language gives the same bits:
 *   no window     a slot with dead[j] != 0 is left alone, and so is a live slot whose w_lo == 0:
 *                 "no window in this cell" (MCNP's convention)
 *   roulette      w < w_lo: (rn0, .) = generate_random_numbers(pkey = pid_base + j, master_key =
 *                 seed, counter 0).  The history survives iff fl(rn0 * w_s) < w -- the form the
 *                 collision kernels' roulette uses -- and goes on with weight w_s; otherwise
 *                 dead = 1, weight = 0.0 and every other field stays as it is
 *   split demand  w > w_hi: q = fl(w / w_hi), m = min(max_split, ceil(q)).  m can be 1 when w is an
 *                 ulp over the bound: the slot is then untouched.  The slot demands e_j = m - 1
 *                 copies (0 for every other slot)
 *   supply        the free slots f_0 < f_1 < ... < f_{F-1}: the slots dead going in and the slots
 *                 this call's roulette has just killed.  A free slot never demands anything
 *   matching      in index order: D_j = e_0 + ... + e_{j-1} (64-bit), copy i = 1 .. e_j of j is
 *                 request r = D_j + i - 1 and goes to slot f_r when r < F.  g_j = clamp(F - D_j, 0,
 *                 e_j) copies are granted to j: when supply runs out the first demanders in index
 *                 order are served, one of them possibly in part;
 *                 copies_refused = max(0, total demand - F)
 *   result        j and its g_j copies all get weight fl(w / (double)(1 + g_j)); a copy is j's other
 *                 nine fields bit for bit, with dead = 0; a history with g_j = 0 is untouched
 * A split conserves weight up to that one rounding, roulette conserves it in expectation.  A
 * particle's random stream is keyed by its slot, so a copy is an independent history from the next
 * step on.  No other slot is touched, in any field, not even in bits that are NaN.
 * With upper_ratio >= 2 a granted split lands inside the window (w / m >= w_hi / 2 >= w_lo), and
 * so does a survivor (w_lo <= w_s <= w_hi).  Hence: when supply suffices and max_split does not
 * bind, a second call with any seed is the identity.
 * Which seeds are safe: as for the fixed source; this project's Python wrapper and driver pass
 * 2^63 + 2^62 + tt, which no timestep (tt), injection (0) or source (2^63 + tt) uses -- the
 * source's counter-0 draw under the same key placed the particle this draw would judge.
 * Returns 0: done -- also when nothing needed doing; when nothing is written a tiled store is not
 * invalidated and the next step pays no re-import, as for the source.  1: nothing changed --
 * particles or lower is NULL, n <= 0, nx or ny < 1; upper_ratio or survival_ratio is not finite,
 * upper_ratio < 2, survival_ratio outside [1, upper_ratio], max_split outside 2 .. 64; or, found
 * on the device before anything is written: a live slot has a cell outside the mesh, a weight that
 * is negative or not finite, or a lower entry that is negative or not finite.  2: nothing changed
 * -- the store is decomposed, as for the comb.
 * Several ranks sharing the mesh: each rank windows its own shard -- its n, its free slots, its
 * keys through pid_base; lower is the replicated global mesh.  Works the same for every kernel
 * variant: pending record state of the tiled variant is written back first (lazy export
 * included), and after a call that wrote the records are dropped, so that the next step imports
 * the arrays again -- slots of the tiled pipeline's graveyard included.
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked slot for slot, bit for bit, against a numpy restatement of this definition, and inside a
 * run against the CPU oracle (tests/test_window.py). */
typedef struct {
  uint64_t live_before, dead_before;
  uint64_t below;              /* live histories under their cell's lower bound */
  uint64_t roulette_killed, roulette_survived;
  uint64_t above;              /* live histories over their cell's upper bound with m >= 2 */
  uint64_t split;              /* of those, the ones granted at least one copy */
  uint64_t copies_made;        /* slots refilled with copies */
  uint64_t copies_refused;     /* copies asked for that found no free slot */
  double roulette_weight_lost, roulette_weight_gained;  /* as NeutralHipStepStats has them */
  double window_ms;            /* HIP-event time of the call's kernels */
} NeutralHipWindowStats;

int neutral_hip_window_particles(NeutralHipParticle* particles, int nparticles,
                                 int nx, int ny, const double* lower /* [device] ny*nx */,
                                 double upper_ratio, double survival_ratio, int max_split,
                                 uint64_t seed, NeutralHipWindowStats* stats /* may be NULL */);

/* ---- census tally: where the live histories and their weight sit, cell by cell --------
 * Every other tally is a step estimator (track length, collision, surface).  This one looks at
 * the store as it stands between two solve_transport_2d calls, in one pass on the device: per
 * cell, how many live histories there are and how much weight they carry -- the diagnostic of
 * population control, and the input of neutral_hip_window_bounds below.
 * With n = nparticles (for a sharded store created by inject_particles: the shard's count, exactly
 * as neutral_hip_comb_particles chooses it): a slot with dead[j] != 0 is skipped and none of its
 * other fields is used (its cell never indexes the mesh).  A live slot j with c = celly[j] * nx +
 * cellx[j] (global cell numbers, ny rows of nx) scores
 *     device_out[c] += 1.0                 a count held in a double: exact
 *     device_out[nx * ny + c] += weight[j] raw: no 1/N, the window's units
 * A SNAPSHOT, NOT AN ACCUMULATOR: unlike the step tallies, which add to what the caller's mesh
 * holds, the call zeroes device_out first.  Nothing is written to the store, so a tiled store is
 * not invalidated and the next step pays no re-import.
 * Reproducibility: the counts are exact, and so is everything derived from them.  A cell's weight
 * is a sum of non-negative doubles in an order the hardware chooses (f64 atomics): with m terms it
 * lies within (m - 1) * 2^-53 * S of the exact sum S (the first-order bound of any summation
 * tree), and it is bit-reproducible from call to call only where every partial sum is exact.
 * Returns 0: done -- also when every slot is dead: zero meshes, occupied_cells 0.  1: nothing
 * usable -- particles or device_out is NULL, n <= 0, nx or ny < 1; or, found on the device in the
 * same pass, a live slot has a cell outside the mesh or a weight that is negative or not finite:
 * such a slot scores nothing, and device_out then holds zeros.  2: the store is decomposed, as for
 * the comb.
 * Several ranks sharing the mesh: each rank tallies its shard; the two meshes are then summed over
 * the ranks on the device (the route of neutral_hip_comm_allreduce_f64), the refusal riding along
 * as one more double, so every rank returns the same code and holds the same meshes.  EVERY RANK
 * MAKES THE CALL (it is collective; the checks of the arguments come out the same on every rank).
 * stats->live and dead are this rank's, the other stats are global.  A rank whose shard is empty
 * (fewer particles than ranks) makes the call like the others and takes part with zeros: it
 * returns their code and holds their meshes.  (The calls on its own shard -- comb, source, window
 * -- still return 1 there, nothing to work on: the driver and Simulation.auto_window skip them.)
 * Works the same for every kernel variant: pending record state of the tiled variant is written
 * back first (lazy export included).
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked against a numpy restatement (tests/census_reference.py), on stores of its own and inside
 * a run against the CPU oracle (tests/test_census.py). */
typedef struct {
  uint64_t live, dead;        /* slots with dead == 0 / != 0 */
  uint64_t occupied_cells;    /* cells with count > 0 */
  uint64_t max_count;         /* most live histories in one cell */
  double weight;              /* sum of the live weights (summed over the cells' sums) */
  double max_cell_weight;     /* M: the largest per-cell weight sum */
  double census_ms;           /* HIP-event time of the call's kernels */
} NeutralHipCensusStats;

int neutral_hip_census_tally(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                             double* device_out /* [device] 2*nx*ny */,
                             NeutralHipCensusStats* stats /* may be NULL */);

/* ---- window bounds: a mesh of lower bounds from a census tally ------------------------
 * neutral_hip_window_particles takes a mesh of lower bounds; this call makes one from a run, by
 * the Cooper-Larsen rule for global problems: the target weight of a cell is proportional to the
 * weight density there, so that every occupied cell ends up with about the same number of
 * histories.  It touches no store and knows no shard.  census is what neutral_hip_census_tally
 * wrote: count_c = census[c], W_c = census[nx * ny + c].  Every step is ONE IEEE f64 operation, in
 * this order, so that a restatement in another language gives the same bits from the same census:
 *   eligible(c)   count_c >= min_count and W_c > 0
 *   K, M          the number of eligible cells; the largest W_c among them (exact, whatever the order)
 *   peak          a = fl(2.0 * (double)K), b = fl(a * M), d = fl(fl(1.0 + upper_ratio) *
 *                 target_population), peak = fl(b / d)
 *   eligible c    r = fl(W_c / M), lower_out[c] = fl(fmax(r, floor_ratio) * peak)
 *   other cells   lower_out[c] = 0.0: the window's "no window in this cell"
 * Why peak: a window [lower, U * lower] settles a cell's histories at about the middle of it,
 * lower * (1 + U) / 2 each, hence W_c / (lower_c * (1 + U) / 2) of them.  With lower_c = peak * W_c
 * / M that is 2 M / (peak * (1 + U)) in every cell alike, and K cells hold target_population when
 * peak = 2 K M / ((1 + U) * target_population).  floor_ratio keeps the bound of a nearly empty
 * cell from falling under floor_ratio * peak (such cells then hold fewer histories).
 * Returns 0: done.  1: lower_out is untouched -- a pointer is NULL, nx or ny < 1,
 * target_population or upper_ratio is not finite, target_population <= 0, upper_ratio < 2,
 * floor_ratio outside [0, 1], min_count < 1; or, found on the device: a census entry is negative
 * or not finite, or no cell is eligible (K == 0).
 * (The ABI version stays 12: detect it by the symbol.)
 * Checked bit for bit against the restatement, and in a loop of census, bounds and window
 * (tests/test_census.py). */
typedef struct {
  uint64_t windowed_cells;   /* K: cells that received a bound > 0 */
  uint64_t floored_cells;    /* of those, the ones held up by floor_ratio: fl(W_c / M) < floor_ratio */
  double max_cell_weight;    /* M */
  double lower_at_peak;      /* the bound of the cell that holds M */
  double bounds_ms;          /* HIP-event time of the call's kernels */
} NeutralHipBoundsStats;

int neutral_hip_window_bounds(int nx, int ny, const double* census /* [device] 2*nx*ny */,
                              double target_population, double upper_ratio, double floor_ratio,
                              int min_count, double* lower_out /* [device] nx*ny */,
                              NeutralHipBoundsStats* stats /* may be NULL */);

/* ---- energy groups for the census tally and the weight window ---------------------------
 * The sources give a run an energy spectrum, and the cross sections span ten decades: in one cell a
 * 1 keV history and a 1 MeV history have very different prospects.  These two calls key the census
 * and the window on (cell, energy group) where the plain calls key them on the cell alone.
 * Groups: ngroups = G in 1 .. 64 and edges[0 .. G], a host array; every edge finite and > 0, the
 * edges strictly ascending (the rule of neutral_hip_set_spectrum_tally).  The group of an energy E
 * is g(E) = #{ i in 0 .. G : edges[i] <= E } - 1 -- comparisons only, nothing to round.  A slot is
 * INSIDE iff 0 <= g < G; otherwise it is OUTSIDE, written g = G.  An energy exactly on an edge
 * belongs to the group above it; E == edges[G] is outside, and so are energies below edges[0],
 * -0.0, negative values, +inf and NaN (for NaN the count is 0: g = -1).  Being outside is not a
 * refusal.
 * Layout: bin b = g * nx * ny + celly * nx + cellx -- G meshes back to back, as the outflow tally
 * lays out its four.  lower has G * ny * nx doubles; the census's device_out has 2 * G * nx * ny: the
 * counts of all bins, then the weights of all bins.  That is exactly a census of a mesh of nx by
 * G * ny, so neutral_hip_window_bounds(nx, G * ny, census, ...) makes the Cooper-Larsen bounds over
 * the (cell, group) bins as it stands: K and M are taken over all bins, and the result is about the
 * same number of histories in every occupied bin.  There is no grouped bounds call.
 * Definition by equivalence.  Make a VIRTUAL STORE in which slot j sits in row g_j * ny + celly[j]
 * of a mesh of nx by (G + 1) * ny, and let block G of lower be zeros.  The grouped window is
 * neutral_hip_window_particles on that store with that mesh, celly put back afterwards.  Every rule
 * of the plain window carries over unchanged: the one IEEE operation per step of its definition;
 * roulette on counter 0 of the stream (pid_base + j, seed); demand, supply and matching in index
 * order; a copy taking the source's nine fields (its energy, hence its group, among them); no other
 * slot touched in any bit.  Every live slot is checked, inside or outside: a cell off the mesh of
 * nx by ny, or a weight that is negative or not finite, refuses the call before anything is written.
 * A lower entry is checked only where a live inside slot looks it up, as the plain window checks
 * only the cells that hold a live slot.  An outside slot has no window: it is left alone and counted
 * in `outside`.
 * The grouped census is neutral_hip_census_tally on the same virtual store with block G dropped:
 * outside slots score nowhere; they are counted in live and in outside, and not in weight,
 * occupied_bins or the maxima.  It remains a snapshot, zeroed first, and collective over ranks
 * that share a mesh: one all-reduce carries 2 * G * nx * ny + 1 doubles, the flag riding last; a
 * rank with an empty shard takes part with zeros.  live, dead and outside are this rank's.
 * Return codes as the plain calls (on a refusal found on the device the stats hold what the plain
 * calls' hold, and outside stays 0).  1 also covers ngroups outside 1 .. 64, NULL edges, an invalid
 * edge, and nx * ny * G > 0x3fffffff.  2: the store is decomposed.  A call that writes nothing
 * leaves a tiled store's records valid; the census never writes to the store.
 * (The ABI version stays 12: detect the calls by their symbols.)
 * Checked against the plain calls on the uploaded virtual store, bit for bit, against the numpy
 * restatements applied to it, and inside a run against the CPU oracle (tests/test_group_window.py). */
typedef struct {
  uint64_t live, dead;      /* this rank's */
  uint64_t outside;         /* this rank's live slots in no group */
  uint64_t occupied_bins, max_count;
  double weight, max_bin_weight, census_ms;
} NeutralHipGroupCensusStats;                                  /* 64 bytes */
typedef struct { NeutralHipWindowStats window; uint64_t outside; } NeutralHipGroupWindowStats; /* 104 */

int neutral_hip_census_tally_groups(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                    int ngroups, const double* edges /* [host] ngroups + 1 */,
                                    double* device_out /* [device] 2*G*nx*ny */,
                                    NeutralHipGroupCensusStats* stats /* may be NULL */);
int neutral_hip_window_particles_groups(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                        int ngroups, const double* edges /* [host] ngroups + 1 */,
                                        const double* lower /* [device] G*ny*nx */,
                                        double upper_ratio, double survival_ratio, int max_split,
                                        uint64_t seed, NeutralHipGroupWindowStats* stats /* may be NULL */);

/* ---- a coarse window mesh: census and window over blocks of cells -------------------------
 * On a sparse problem -- a mesh of 4000 x 4000 cells under 1e6 histories is 0.06 per cell -- a
 * census per transport cell finds 0 or 1 history almost everywhere, and bounds made from it window
 * nothing.  Production weight windows live on a superimposed mesh coarser than the transport mesh.
 * These two calls key the census and the window on blocks of block_x by block_y cells, with or
 * without energy groups.
 * Bins: cnx = ceil(nx / block_x), cny = ceil(ny / block_y); the last block of a row or column may
 * be narrower.  ngroups = G in 0 .. 64; G = 0 is "no groups" and takes edges = NULL, G >= 1 takes
 * edges as the grouped calls do.  B = max(G, 1) * cnx * cny bins,
 *   bin = g * cnx * cny + (celly div block_y) * cnx + (cellx div block_x)   (g = 0 without groups):
 * max(G, 1) coarse meshes back to back.  lower has B doubles, device_out 2 * B: the counts of all
 * bins, then their weights.  That is a census of a mesh of cnx by max(G, 1) * cny, so
 * neutral_hip_window_bounds(cnx, max(G, 1) * cny, census, ...) makes the bounds over the bins as it
 * stands.  There is no blocks bounds call.
 * Definition by equivalence.  First every live slot is checked on the REAL store: a cell off the
 * mesh of nx by ny, or a weight that is negative or not finite, refuses the call (code 1, nothing
 * written; the census then holds zeros).  The check is on the true cell: with nx = 10 and block_x
 * = 4, cellx = 11 refuses, though 11 div 4 = 2 would be a block of the coarse mesh.  Then make a
 * VIRTUAL STORE in which cellx' = cellx div block_x and celly' = celly div block_y, on a mesh of cnx
 * by cny.  The call is neutral_hip_census_tally / neutral_hip_window_particles (G = 0) or
 * neutral_hip_census_tally_groups / neutral_hip_window_particles_groups (G >= 1) on that store with
 * that mesh, cellx and celly put back afterwards; a copy takes its source's TRUE cell with the other
 * fields.  Everything else carries over unchanged: the one IEEE operation per step; roulette on
 * counter 0 of the stream (pid_base + j, seed); demand, supply and matching in index order;
 * `outside`; a lower entry checked only where a live inside slot looks it up; no other slot touched
 * in any bit; a call that writes nothing leaves a tiled store's records valid.  The census is a
 * snapshot, zeroed first, and collective over ranks that share a mesh: one all-reduce carries
 * 2 * B + 1 doubles.  The window works per shard.  With block_x = block_y = 1 the calls are the
 * plain (G = 0) or the grouped calls bit for bit.
 * Return codes as the grouped calls.  1 also covers block_x or block_y < 1, ngroups outside 0 .. 64,
 * ngroups > 0 with NULL or invalid edges, ngroups == 0 with edges that are not NULL (a caller's
 * mistake: groups forgotten), and B > 0x3fffffff.  2: the store is decomposed.
 * privatised: 1 when the census's pass over the store summed each workgroup's bins in LDS and added
 * only the non-empty ones to memory, 0 when every live slot added to memory itself.  The pass takes
 * the LDS form where B is at most 4096; NEUTRAL_CENSUS_LDS_BINS in the environment, read at every
 * call, sets another limit at or below that (0: never).  The counts do not depend on the form; the
 * weights are sums in another order.  Without groups, outside is 0.
 * (The ABI version stays 12: detect the calls by their symbols.)
 * Checked against the plain and grouped calls on the uploaded virtual store, bit for bit, against
 * the numpy restatements applied to it, and inside a run against the CPU oracle
 * (tests/test_block_window.py). */
typedef struct {
  NeutralHipGroupCensusStats census;
  uint64_t privatised;
} NeutralHipBlockCensusStats;                                  /* 72 bytes */

int neutral_hip_census_tally_blocks(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                    int block_x, int block_y,
                                    int ngroups, const double* edges /* [host] ngroups + 1; ngroups 0 and NULL: no groups */,
                                    double* device_out /* [device] 2 * B */,
                                    NeutralHipBlockCensusStats* stats /* may be NULL */);
int neutral_hip_window_particles_blocks(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                        int block_x, int block_y,
                                        int ngroups, const double* edges /* as above */,
                                        const double* lower /* [device] B */,
                                        double upper_ratio, double survival_ratio, int max_split,
                                        uint64_t seed, NeutralHipGroupWindowStats* stats /* may be NULL */);

/* ---- in-step weight window: roulette by the window's mesh -----------------------------
 * The census window sees a weight only after it has fallen through a step's absorptions, and
 * neutral_hip_set_roulette knows one cutoff for the whole mesh.  This call puts a window's lower
 * bounds in force INSIDE the steps: the game is neutral_hip_set_roulette's, with the cutoff taken
 * per bin.  Splitting stays at the census (the store has a fixed size).
 * lower is what neutral_hip_window_particles, ..._groups and ..._blocks take: the GLOBAL mesh,
 * replicated on every rank.  ngroups = 0 with edges = NULL means no groups, block_x = block_y = 1 no
 * blocks.  With cnx = ceil(nx / block_x) and cny = ceil(ny / block_y), lower holds
 * max(ngroups, 1) * cnx * cny doubles, and the bin of a collision is
 *   g * cnx * cny + (celly div block_y) * cnx + (cellx div block_x)
 * where cellx, celly are the global numbers of the cell the history collides in and g is the group
 * of the energy it has as it collides (an absorption does not change the energy).  The group is
 * found as the census calls find it: comparisons only; on an edge, the group above; below edges[0],
 * at or above edges[G], or NaN: no group.
 * The game:
 *   - only inside an absorption, after the weight has dropped to w = weight * (1 - p_absorb), and
 *     after the energy-death rule, which comes first and plays none;
 *   - w_lo = lower[bin]; the history plays iff w < w_lo, so a bound of 0.0 is "no window in this
 *     bin", as for the census window, and so is "no group";
 *   - the sample is the second number of the absorption's own draw, rn1[1]: the counter schedule
 *     does not change;
 *   - w_s = fl(survival_ratio * w_lo); the history survives iff fl(rn1[1] * w_s) < w and goes on at
 *     weight w_s; otherwise it dies exactly as a roulette death does: dead = 1, its pending scores go
 *     to its cell, its stored weight becomes 0.0;
 *   - every operation is one IEEE f64 operation, kept out of contraction, the same in both
 *     arithmetic policies.
 * Consequences: a history's path is bit for bit its path with roulette off, up to where it is
 * killed.  A uniform mesh of value c with ratio r gives the bits of neutral_hip_set_roulette(c,
 * fl(r * c)) in every array, tally and counter.  A mesh of zeros gives the bits of a run with nothing
 * set.  Blocks of 1 x 1 give the bits of the plain form, and so does one group that contains every
 * energy; a blocks mesh gives the bits of the plain form on the same mesh expanded to cells.
 * What the game did is reported where roulette's is: NeutralHipStepStats.roulette_killed,
 * roulette_survived, roulette_weight_lost and roulette_weight_gained, summed over the ranks.
 * The setting persists across steps.  lower == NULL turns it off: that touches no device, and the
 * other arguments are ignored.  The library reads the caller's mesh at every absorption: the buffer
 * must stay allocated while set, and may be rewritten between steps (neutral_hip_window_bounds into
 * the same buffer is the intended use).  The edges are copied at the call.  The two roulettes are
 * exclusive: this call returns 1 while a global cutoff is set, and neutral_hip_set_roulette with a
 * non-zero pair returns 1 while a mesh is set ((0, 0) is accepted as ever).
 * Returns 0: set.  1, nothing changed, decided before any device call: nx or ny < 1; survival_ratio
 * not finite or < 1; ngroups outside 0 .. 64; edges NULL with ngroups > 0, not NULL with ngroups == 0,
 * not strictly ascending, not finite or not positive; a block < 1; more than 0x3fffffff bins; a global
 * cutoff in force.  1, nothing changed, found by one small reduction kernel over the mesh at set
 * time: an entry that is negative or not finite.  (A mesh rewritten later is not checked again: a
 * negative or NaN entry never plays, an infinite one always does, with w_s infinite.)
 * A step whose global nx / ny differ from this call's does not run: solve_transport_2d prints a
 * message and exits, like its other argument errors.  Apart from that a cell outside nx by ny has no
 * window, so nothing is ever read outside lower.
 * Several ranks: particle shards and a decomposed mesh both work -- cells are global numbers, the
 * mesh is replicated, and a history handed to another rank carries only its weight.
 * It works with every kernel variant, both arithmetic policies, lazy export, stream queues and every
 * optional tally.  A compile-time property of the kernels that collide, like roulette: with nothing
 * set the kernels that run are the ones without any of this code.
 * (The ABI version stays 12: detect the call by its symbol.)
 * Checked against a Python restatement that is itself pinned to the CPU oracle's roulette, and by
 * the equivalences above (tests/test_window_roulette.py). */
int neutral_hip_set_window_roulette(int nx, int ny, const double* lower /* [device] */,
                                    double survival_ratio,
                                    int ngroups, const double* edges /* [host] ngroups + 1, or NULL */,
                                    int block_x, int block_y);

/* ---- batch statistics: a standard error and a relative error for every tally -----------
 * A tally says nothing of how good it is.  Independent batches do: a store made for the global
 * particles [first, first + count) steps them with their own RNG keys, and every tally is
 * normalised by ntotal_particles, so the tallies of B disjoint shards of the N particles are B
 * independent estimates that add up to the tally of the whole run.  The two calls below keep the
 * running moments of such batches and turn them into an estimate with its relative error, on the
 * device.  They work on ANY array of doubles there -- the energy tally, the scalar flux, the
 * collision tallies, Jx, Jy, the four outflow meshes as one array, a spectrum's 2 * ngroups values
 * -- and know no store, no shard and no rank: with several ranks sharing a mesh every rank holds
 * the same all-reduced tally and computes the same statistics; nothing here is collective.
 *
 * neutral_hip_batch_fold folds batch number k (1-based) into moments[0 .. len) (the means) and
 * moments[len .. 2 * len) (M2, the sums of squared deviations) by Welford's update.  Every step is
 * ONE IEEE f64 operation, in this order, per entry i, so that a restatement in another language
 * gives the same bits:
 *   k == 1:   mean = x, M2 = 0.0         (what moments held is ignored: there is no reset call)
 *   k  > 1:   d = fl(x - mean), mean' = fl(mean + fl(d / (double)k)), d2 = fl(x - mean'),
 *             M2' = fl(M2 + fl(d * d2))
 * Returns 0: done.  1: moments is untouched -- a pointer is NULL, len is 0 or above 2^30, k < 1;
 * or, found on the device before anything is written, an entry of x is not finite.
 * stats->sum is the sum of x in a fixed order (the same bits on every call); within
 * (len - 1) * 2^-53 * sum|x| of the exact sum, like any summation tree.
 *
 * neutral_hip_batch_statistics turns the moments of B = nbatches batches into, per entry:
 *   estimate = fl(scale * mean)              (scale = B: the tally of all B shards together)
 *   var = fl(M2 / (double)(B - 1)), se = sqrt(fl(var / (double)B))   (IEEE sqrt: the standard
 *                                             error of the batch mean)
 *   relerr = mean != 0.0 ? fl(se / fabs(mean)) : 0.0
 * An entry is `scored` when its mean is not 0.0; the counts, the maximum and the mean of relerr are
 * over the scored entries (the two sums in a fixed order, as above).
 * Returns 0: done.  1: both outputs are untouched -- a pointer is NULL, len is 0 or above 2^30,
 * nbatches < 2, scale is not finite and positive; or, found on the device, a mean is not finite,
 * or an M2 is negative or not finite.
 * Neither call reads or writes a particle store: a tiled store's records stay valid and the next
 * step pays no re-import.  (The ABI version stays 12: detect the calls by their symbols.)
 * Checked bit for bit against a numpy restatement (tests/batch_reference.py), and in batched runs
 * against the CPU oracle (tests/test_batches.py). */
typedef struct {
  double sum;         /* the sum of x over its len entries (the same bits on every call) */
  uint64_t nonzero;   /* entries of x that are not 0.0 */
  double fold_ms;     /* HIP-event time of the call's kernels */
} NeutralHipBatchFoldStats;

int neutral_hip_batch_fold(const double* x /* [device] len */, size_t len, int k,
                           double* moments /* [device] 2 * len: means, then M2 */,
                           NeutralHipBatchFoldStats* stats /* may be NULL */);

typedef struct {
  uint64_t scored;        /* entries whose mean is not 0.0 */
  uint64_t within_10pc;   /* of those, relerr <= 0.1 */
  uint64_t within_5pc;    /* of those, relerr <= 0.05 */
  double max_relerr;      /* over the scored entries (exact: a maximum) */
  double mean_relerr;     /* fl(sum of relerr over the scored entries / scored) */
  double estimate_sum;    /* sum of estimate_out */
  double stats_ms;        /* HIP-event time of the call's kernels */
} NeutralHipBatchStats;

int neutral_hip_batch_statistics(const double* moments /* [device] 2 * len */, size_t len, int nbatches,
                                 double scale, double* estimate_out /* [device] len */,
                                 double* relerr_out /* [device] len */,
                                 NeutralHipBatchStats* stats /* may be NULL */);

/* ---- ranks: one process per GPU on one node ------------------------------------
 * The reference leaves rank and rank count to the parent project's initialise_mpi
 * (main.c:62) and calls barrier() (main.c:75,112) and reduce_all_sum
 * (omp3/neutral.c:530); its own MPI code is compiled out (neutral_data.h:10-14).
 * Here ranks are processes started by a launcher that exports RANK, WORLD_SIZE,
 * LOCAL_RANK, MASTER_ADDR, MASTER_PORT (torchrun's convention; `neutral.hip --gpus
 * N` forks them itself).  Particles are sharded over the ranks in contiguous id
 * ranges, the mesh is replicated, and solve_transport_2d ends every timestep with
 * ONE all-reduce of that step's tally contributions (sum, f64, nx*ny) over RCCL /
 * xGMI, after which energy_deposition_tally holds the same global mesh on every
 * rank -- all behind the unchanged three functions:
 *   inject_particles(nparticles = N, ...)  creates this rank's shard of the N
 *       particles (global ids first..first+count-1 as RNG keys);
 *   solve_transport_2d(...)                steps the shard it finds in `particles`
 *       (*nlocal_particles is not rewritten), all-reduces tally and event counters;
 *   validate(...)                          sums the (already global) tally.
 * The unchanged main.c gets there through the host layer linked into this library:
 * initialise_mpi reads the environment, initialise_devices binds the rank to GPU
 * LOCAL_RANK and calls neutral_hip_comm_start(). */
enum {
  NEUTRAL_HIP_COMM_NONE = 0, /* one rank */
  NEUTRAL_HIP_COMM_RCCL = 1, /* ncclAllReduce on the kernels' stream */
  NEUTRAL_HIP_COMM_HOST = 2  /* staged through the host over TCP (RCCL unavailable, or
                                NEUTRAL_HIP_COMM=host: ranks sharing a GPU in tests) */
};
/* Joins the ranks (TCP rendezvous at MASTER_ADDR:NEUTRAL_COMM_PORT, default
 * MASTER_PORT + 1), then brings up RCCL on the current device (select it first) with
 * a time limit (NEUTRAL_COMM_TIMEOUT seconds, default 120).  Returns the transport in
 * use (NEUTRAL_HIP_COMM_*).  Idempotent. */
int neutral_hip_comm_start(void);
void neutral_hip_comm_stop(void);
int neutral_hip_comm_rank(void);
int neutral_hip_comm_nranks(void);
int neutral_hip_comm_transport(void);
/* RCCL's version number as ncclGetVersion reports it (0: librccl is not loadable here) */
int neutral_hip_comm_rccl_version(void);
/* sharding by inject_particles when there are several ranks (default 1); 0 leaves the
 * id range to the caller (neutral_hip_set_pid_base + its own particle count) */
void neutral_hip_set_auto_shard(int on);
/* particles in a sharded or decomposed store created by inject_particles (this rank's
 * share, or what is inside its block right now); -1 for any other store */
int neutral_hip_store_count(const NeutralHipParticle* particles);
/* ---- spatial domain decomposition (mesh too large to replicate) -------------------
 * The reference has the plumbing only: rank offsets and neighbours in the interface
 * (neutral_interface.h:13-15), PARTICLE_SENT (neutral_data.h:35), a
 * send_and_mark_particle that is declared (omp3/neutral.h:63) and never defined; its
 * facet_event walks off the local arrays (omp3/neutral.c:333-377) and its RNG key is
 * the local array index (:89), so a decomposed run of it could not reproduce an
 * undecomposed one.  Here: ranks_x x ranks_y ranks (= the ranks of the rank layer) own
 * uniform blocks of the mesh; solve_transport_2d is called with the block's extent
 * (nx, ny, x_off, y_off, arrays of the block: edges nx+1 / ny+1, density and tally
 * nx*ny, pad = 0) and the global one (global_nx, global_ny).  A history that crosses
 * into another rank's block stops on the facet, is sent there with its RNG counter,
 * and goes on in the same timestep: rounds of exchange (RCCL send/recv; staged through
 * the host otherwise) until no rank has a history in flight.  Keys are global particle
 * ids, so every history is the one an undecomposed run computes, whichever ranks it
 * visits; tallies are per block (validate sums them over the ranks).  Tiled variant
 * only.
 *   neutral_hip_set_decomposition  names the grid (after neutral_hip_comm_start) and
 *       returns this rank's block; 0 on success, 1 if the grid does not match the ranks
 *   neutral_hip_set_source_box     the GLOBAL source box (same numbers on every rank);
 *   inject_particles(nparticles = N, ...) then makes a store with room for all N, holding
 *       the particles the source puts into this rank's block; their number changes as
 *       histories cross: solve_transport_2d writes it to *nlocal_particles, and
 *       neutral_hip_store_count / neutral_hip_store_keys give it and the ids ([device],
 *       keys[i] = id of the particle at index i of the arrays). */
int neutral_hip_set_decomposition(int ranks_x, int ranks_y, int global_nx, int global_ny,
                                  int* x_off, int* y_off, int* local_nx, int* local_ny);
void neutral_hip_clear_decomposition(void);
void neutral_hip_set_source_box(double left, double bottom, double width, double height);
const unsigned* neutral_hip_store_keys(const NeutralHipParticle* particles);

/* in-place sum over the ranks of n doubles in [device] memory, on hip_stream */
void neutral_hip_comm_allreduce_f64(double* device_buf, size_t n, void* hip_stream);
/* max over the ranks of a host scalar; barrier of the ranks (host side) */
double neutral_hip_comm_max(double v);
void neutral_hip_comm_barrier(void);
/* used by the host layer: bind this rank to its GPU and start the rank layer;
 * finish the device's work (the device half of barrier()) */
void neutral_hip_bind_rank_device(int local_rank);
void neutral_hip_comm_barrier_device(void);
/* one-rank RCCL check on the current device: 0 ok, 1 librccl not loadable, 2 failure */
int neutral_hip_comm_selftest(int n);

/* Frees a store created by inject_particles. */
void neutral_hip_free_particles(NeutralHipParticle* particles);
/* Raw copies for callers without a HIP runtime of their own (ctypes, C). */
void neutral_hip_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);
void neutral_hip_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
void neutral_hip_memset(void* dst_device, int value, size_t bytes);
void neutral_hip_synchronize(void);
/* Unit probes of the device building blocks, for known-answer tests.  All
 * pointers are HOST arrays; the library stages them through HBM.
 *   threefry:  in3 = n rows {counter, pkey, master_key}; out2 = n rows of the
 *              two Threefry2x64-20 words; rn2 = the two (0,1] doubles of
 *              generate_random_numbers (omp3/neutral.c:632-652)
 *   cs_lookup: microscopic_cs_for_energy (omp3/neutral.c:498-517) of `cs`
 *              ([device] table) at n energies -> value and bracket index;
 *              use_index = 1 searches through the exponent-bucketed index the
 *              history kernels use, 0 by plain bisection
 *   distance_to_facet: in9 = n rows {x, y, omega_x, omega_y, speed, edgex[c],
 *              edgex[c+1], edgey[c], edgey[c+1]} (omp3/neutral.c:423-471) */
void neutral_hip_probe_threefry(const uint64_t* in3, uint64_t* out2, double* rn2, int n);
void neutral_hip_probe_cs_lookup(const NeutralHipCrossSection* cs, const double* energy,
                                 double* value, int* index, int n, int use_index);
void neutral_hip_probe_distance_to_facet(const double* in9, double* distance, int* x_facet,
                                         int n);
/*   division:  in2 = n rows {a, b}; out2 = n rows {a / b as the compiler divides,
 *              the quotient through the kept reciprocal of b (the stream kernel's
 *              form of omp3/neutral.c:311-312)}; plain[i] = 1 when both operands lie
 *              in the range where the kernel uses the second form */
void neutral_hip_probe_division(const double* in2, double* out2, int* plain, int n);
/*   log:       out8 = n rows {the logarithm the history kernels take of a sample
 *              (omp3/neutral.c:131,295), the device library's log, the kernels'
 *              square root (:255-259,297), the compiler's sqrt} of x[i], followed by
 *              n rows {x / PARTICLE_MASS the kernels' way (:297), as the compiler
 *              divides, x / (MASS_NO+1)^2 the kernels' way (:252), as the compiler
 *              divides} */
void neutral_hip_probe_log(const double* x, double* out8, int n);
/*   scatter:   in4 = n rows {energy, the centre-of-mass cosine mu, omega_x, omega_y}; out10 = n rows
 *              {the energy after the scatter (omp3/neutral.c:257-259), the laboratory cosine
 *              (:263-265) the fast kernels' way and with the compiler's divisions and roots, the
 *              speed after the scatter (:297) from the speed before it and as sqrt(2 E' eV / m),
 *              1 / (omega_x speed) and 1 / (omega_y speed) (:435-436) off one reciprocal and as
 *              two divisions, the laboratory cosine the checked kernels' way}: what the fast
 *              arithmetic policy seeds from its neighbours */
void neutral_hip_probe_scatter(const double* in4, double* out10, int n);
/*   policy_quotient: in2 = n rows {a, b}; out8 = n rows {a / b as the compiler divides, the
 *              kernels' quotient of physical operands fast and checked, the stream kernel's two
 *              facet quotients (:311-312: b as mean free path, b as speed) through reciprocals
 *              kept as the fast kernels keep them, the same as the checked kernels keep them,
 *              v_rcp_f64(b)}
 *   policy_root: in2 = n rows {x, energy}; out10 = n rows {sqrt(x) as the compiler takes it,
 *              the kernels' root of a physical argument fast and checked, of 1 - cos^2 (:266)
 *              fast and checked, v_rsq_f64(x), the speed sqrt(2 E eV / m) (:116,297) fast and
 *              checked, the fast speed's argument, v_rsq_f64 of that argument} */
void neutral_hip_probe_policy_quotient(const double* in2, double* out8, int n);
void neutral_hip_probe_policy_root(const double* in2, double* out10, int n);
/* Library/ABI version, bumped on any signature change. */
int neutral_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
