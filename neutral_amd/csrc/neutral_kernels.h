/*
 * neutral_kernels.h -- launch-side view of the HIP kernels (host code of the
 * C-ABI includes this; kernels are defined in neutral_kernels.hip).
 */
#ifndef NEUTRAL_AMD_KERNELS_H
#define NEUTRAL_AMD_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neutral_window_bins.h"

namespace neutral {

/* SoA particle store in HBM: the reference's -DSoA Particle
 * (neutral_data.h:45-61).  One f64/i32 stream per field, lane i <-> particle
 * base+i, so every prologue/epilogue access is a fully coalesced 512-B (f64) or
 * 256-B (i32) wave transaction. */
struct ParticleView {
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
};

/* One particle as a record: the private working layout of the tiled variant.
 * Sorted-by-tile access is random per particle, and a random 80-B record costs
 * two 64-B sectors where the SoA store costs eleven; the records are kept in
 * tile order from step to step and carry the particle id (the RNG key). */
/* What a history that neither collides nor reflects changes comes FIRST (48 bytes: position, the
 * two clocks, cell, id, state): the write-back of such a history reads those three quads -- one
 * 64-byte sector for every other record instead of two -- and stores six fields, not eleven
 * (export_records_kernel; the state word says whether direction, energy or weight changed). */
struct alignas(16) ParticleRec {
  double x, y, dt_to_census, mfp_to_collision;
  int cellx, celly;
  unsigned id; /* index in the SoA store = global id - pid_base */
  int dead;    /* the record's state word: neutral_history.h, record_word() */
  double omega_x, omega_y, energy, weight;
};
constexpr int kParticleRecBytes = 80;
static_assert(sizeof(ParticleRec) == kParticleRecBytes, "ParticleRec holds 80 bytes");

/* What a history suspended MID-CHAIN by the collision stage's time slicing needs
 * beyond its record: the RNG counter, the deposition not yet tallied
 * (omp3/neutral.c:236: flushed only at a facet, the census or death) and the
 * watchdog count.  Indexed like the record array. */
struct alignas(16) SuspendExtra {
  double energy_deposition;
  unsigned counter;
  unsigned nevents;
};
/* (with the scalar-flux tally the pending weight * path length of such a history
 * lives in a parallel array of doubles: TiledArgs::susp_track) */

/* what the start of a history does not depend on (TiledArgs::carried_in) */
struct alignas(16) CarriedStart {
  double micro;          /* microscopic cross section of the record's energy (identical tables) */
  double minus_log_rn0;  /* -log of the timestep's first sample (omp3/neutral.c:127-131) */
};

struct InjectArgs {
  int nparticles;
  uint64_t pid_base;
  int local_nx;
  int local_ny;
  int pad;
  int x_off;
  int y_off;
  double left_off;
  double bottom_off;
  double width;
  double height;
  double dt;
  double initial_energy;
  const double* edgex;
  const double* edgey;
  ParticleView p;
};

/* device-resident event counters of one solve step */
struct StepCounters {
  unsigned long long nprocessed;
  unsigned long long nfacets;
  unsigned long long ncollisions;
  unsigned long long ncensus; /* histories that ended in a census event */
  unsigned int queue_head;    /* K2: next unclaimed particle index */
  unsigned int aborted;       /* histories stopped by the event watchdog (should be 0) */
  unsigned long long nrequeued; /* time-slice swaps of the collision stage (queue mode) */
  unsigned long long ncollide_passes; /* wave-level COLLIDE passes of the regroup kernel */
  unsigned long long nsteals; /* collision stage: rings a wave took half the waiting histories of */
  unsigned long long steal_refused; /* collision stage: waves that found a CU list of more than
                                       kCuWavesMax entries and therefore stole nothing (the key
                                       read from the hardware does not name one CU: see StealWork) */
  unsigned long long nweighted; /* collision stage: waves that were dealt a share in proportion to
                                   what a wave is served (SolveArgs::share_weight) */
  /* The shader clock the kernel ran at, measured by one wave of every launch over its own
   * life: ticks of the shader clock (s_memtime) and of the constant 100-MHz clock
   * (s_memrealtime), summed over the step's launches.  The chip does not hold its nominal
   * 2.4 GHz under every load (a kernel of nothing but v_fma_f64 runs at 1.85 GHz:
   * profiles/r05/pmc_calibration.log), and a roofline in issue cycles needs the clock there was. */
  unsigned long long clock_shader_ticks;
  unsigned long long clock_100mhz_ticks;
  unsigned long long clock_parked[2]; /* (the measuring wave's counters at its start) */
  /* Russian roulette (neutral_hip.h: neutral_hip_set_roulette; zero when it is off): the
   * histories it killed and kept, the weight w the killed had, the w_s - w the kept gained.
   * (Last: the fields above keep their offsets, and the kernels without roulette their code.) */
  unsigned long long roulette_killed;
  unsigned long long roulette_survived;
  double roulette_weight_lost;
  double roulette_weight_gained;
  /* Vacuum sides (neutral_hip.h: neutral_hip_set_vacuum_sides; zero when none is): the histories
   * that escaped through each outer side, numbered as the outflow tally numbers them, and the sum
   * of the weights they left with.  (Behind everything else, for the same reason.) */
  unsigned long long escaped[4];
  double escape_weight[4];
  /* Periodic axes (neutral_hip.h: neutral_hip_set_periodic_axes; zero when none is): the histories
   * that wrapped through each outer side -- the side they LEFT through, numbered likewise -- and the
   * sum of the weights they wrapped with.  (Last of all, for the same reason.) */
  unsigned long long wrapped[4];
  double wrap_weight[4];
};

/* Device workspace of the collision stage's work stealing (neutral_kernels.hip): the control
 * word of every wave's ring, who is reading from which ring, and the list of waves per CU key.
 * It belongs to the tiled workspace (TiledArgs::steal), is handed to the kernel in SolveArgs and
 * is reset by one kernel on the launch's own stream before every collision stage. */
constexpr int kRingCtlSlots = 8192;  /* waves of a launch (4 096 on an MI355X) */
constexpr int kCuSlots = 4096;       /* (xcc 4 bits, se 3, sh 1, cu 4) */
/* (16 waves of a launch are resident on a CU at a time, but a key can collect more over a launch's
 * life: the write-back pass that starts beside the collision stage may hold wave slots when the
 * stage's workgroups are placed, the ones left over are placed when a slot frees up -- also on a
 * CU whose first workgroups have gone through their small shares and left, where they are the
 * fifth to enter themselves.  Twice a CU's waves: a key that collects more does not name a CU) */
constexpr int kCuWavesMax = 32;
struct StealWork {
  unsigned long long ring_ctl[kRingCtlSlots]; /* head << 32 | waiting */
  /* waves that are reading entries out of a ring they have just taken from: the owner waits
   * for zero before it writes into its ring (hand-back) or re-uses it for what it steals */
  unsigned ring_readers[kRingCtlSlots];
  unsigned cu_count[kCuSlots];
  unsigned cu_members[kCuSlots * kCuWavesMax];
  unsigned overfull; /* a CU key collected more than kCuWavesMax waves: nobody steals */
};

struct SolveArgs {
  int nx;
  int ny;
  int global_nx;
  int global_ny;
  uint64_t master_key;
  int pad;
  int x_off;
  int y_off;
  double dt;
  double inv_ntotal_particles;
  int nparticles;
  uint64_t pid_base;
  ParticleView p;
  const double* density;
  const double* edgex;
  const double* edgey;
  /* The mesh as a formula, when it is one: edge[pad + i] == edge_d * (double)(off + i), bit
   * for bit, for every edge of both axes (the way the reference's host layer makes uniform
   * meshes: edgedx[i] * (x_off + i - pad)).  The spacings are read once per mesh from the
   * caller's edgedx / edgedy (0: none given); whether the formula HOLDS is checked on the
   * device every step (TiledArgs::edges_computed), and the stream kernel then works the two
   * edges of a crossing out instead of loading them. */
  double edge_dx;
  double edge_dy;
  const double* scatter_keys;
  const double* scatter_values;
  int scatter_n;
  const double* absorb_keys;
  const double* absorb_values;
  int absorb_n;
  int same_tables; /* both tables have identical contents: search once */
  int checked;     /* arithmetic policy of the event bodies (neutral_device.h): 0 the fast
                      sequences, proven on densities and table entries in [2^-100, 2^100];
                      1 IEEE operations with range tests, any input the reference accepts */
  /* exponent-bucketed indexes over the key arrays (start == null: none) */
  const unsigned short* scatter_index;
  int scatter_index_n;
  long long scatter_index_base;
  const unsigned short* absorb_index;
  int absorb_index_n;
  long long absorb_index_base;
  int index_shift;
  double* tally;
  double* flux_tally; /* scalar-flux tally (null: not kept; see neutral_hip.h) */
  StepCounters* counters;
  /* optional work list for the regroup kernel: ids of particles another kernel
   * suspended at their first collision (null: all particles 0..nparticles-1) */
  unsigned* queue;           /* (the collision stage re-uses its words as per-wave rings) */
  const unsigned* queue_len; /* [device] number of valid entries */
  ParticleRec* rec;          /* queue entries index this record array (tiled variant) */
  int blocks_per_cu;         /* > 0: cap on the regroup kernel's workgroups per CU; -1: the
                                collision stage picks 1..3 itself from its queue length */
  int max_blocks;            /* > 0: cap on the regroup kernel's grid (test knob) */
  unsigned* slot_info;       /* per-record summary kept next to rec (see TiledArgs) */
  int tiles_x;               /* tiles per mesh row, for the summary's tile field */
  int tile_shift;            /* log2 of the tile edge in cells (4..7) */
  SuspendExtra* susp;        /* per-record side store of time-sliced histories (queue mode) */
  double* susp_track;        /* ... their pending weight * path length (scalar flux only) */
  CarriedStart* carried;     /* per-record microscopic cross section the collision stage leaves for
                                the next timestep's start (TiledArgs::carried_out; null: not kept) */
  int steal_min;              /* collision stage: waiting histories a ring must hold to be taken
                                 from by a CU-mate (0: no stealing; NEUTRAL_STEAL_MIN) */
  StealWork* steal;           /* [device] rings' control words and CU lists (null: no stealing) */
  int steal_delay;            /* test knob: sleeps of a thief between its take and its copy
                                 (NEUTRAL_STEAL_DELAY; 0 in production) */
  int occupancy_rows;         /* collision stage: workgroups per CU resident together, among
                                 which the kernel picks how many work (0: all) */
  int share_weight;           /* collision stage: how many times the others' share of the queue
                                 the waves of the launch's first row of workgroups start with (the
                                 oldest wave of a SIMD is served first; 1: equal shares) */
  int weighted_share_min;     /* ... from this many histories per wave on (equal shares below) */
  int compute_units;          /* CUs of the device the launch goes to (read once per store) */
  int export_skip_long_dead;  /* the arrays were current as the step began: particles dead
                                 since before it are left alone by the write-back pass */
  /* [device] the SoA store's array pointers, when the collision stage writes the final state
   * of every history it ends to the arrays itself -- so that the write-back of everybody else
   * can run beside it (TiledArgs::susp_ids; null: it does not).  Read where a history ends,
   * not held in registers through the collision loop. */
  const ParticleView* export_view;
  /* spatial domain decomposition: this rank owns cells [x_off, x_off + nx) x [y_off,
   * y_off + ny) of a larger mesh; a history that crosses out of them is stored as an
   * emigrant instead of going on (0: the rank owns the whole mesh) */
  int decomposed;
  unsigned* emigrants; /* [device] their count (collision stage; the stream kernel has t.ctrl) */
  /* [device] non-zero: the host's cached view of the cs tables (identity, bucketed
   * indexes) no longer matches the tables; history kernels return at once and the
   * host re-runs the step with a fresh view (null: no cached view in use) */
  const int* abort_flag;
  /* (no collision tallies here: see StepOptions) */
};

/* device workspace of the tiled pipeline (neutral_tiled.hip), owned by the ABI */
struct TiledArgs {
  ParticleRec* rec_in;     /* nparticles: last step's records (source of pass 0) */
  ParticleRec* rec_out;    /* nparticles: this step's records, in this step's tile order */
  /* 4-B summary of each record, written with it: state << 29 | tile of its cell.
   * The counting sort and the collision queue are built from these 4 bytes instead
   * of a strided read of the 80-B records. */
  unsigned* info_in;
  unsigned* info_out;
  unsigned* id_in;         /* nparticles: particle id of each record (= rec.id, kept apart so */
  unsigned* id_out;        /* that a reader takes 4 bytes per record, not a 64-byte sector) */
  unsigned* slot_of_id;    /* nparticles: where particle id's record is -- what the write-back
                              goes by */
  /* What a history's start does not depend on, kept per record slot so that the stream kernel
   * starts from it (CarriedStart above; neutral_history.h: prologue_carried; identical tables, one
   * rank's whole mesh, no tile queues -- the other instantiations look up and draw as before):
   * carried_in / carried_out next to rec_in / rec_out.  `micro` is written by whoever places the
   * record (pass 0 of the stream kernel copies it across) or changes its energy (the collision
   * stage, where it ends a history), and is valid for every live slot of rec_in whenever the host
   * says so (it runs refresh_micro_kernel first when not: a store just imported, a table view
   * just rebuilt); `minus_log_rn0` of carried_in is worked out by the counting sort's placement
   * pass (pass 0) from id_in.  One 16-byte pair per slot: the stream kernel's gather is one
   * 64-byte sector per history beside the record's two, not two (the split deck, whose stream
   * kernel is nothing but refills, ran 6 % slower with two arrays: profiles/r05/experiments). */
  CarriedStart* carried_in;
  CarriedStart* carried_out;
  int carried;             /* 1: this step's stream kernel starts from them (set per step) */
  /* The graveyard.  Records [sort_end, nparticles) belong to particles that were dead when
   * the LAST step began: they keep their slots for good, in both record buffers, and take
   * no part in the sort.  The dead of this step's sort are carried over to [first_inactive,
   * sort_end) of rec_out by copy_inactive (and become graveyard next step); those carried
   * over last step, [sort_end, mirror_end), are so far in rec_in only and are copied across
   * once.  A dead particle thus costs two record copies, not one per step.  Decomposed
   * stores (whose slot population changes within a step) keep sort_end = mirror_end =
   * nparticles. */
  int sort_end;
  int mirror_end;
  int slots_by_id;         /* 1: the kernels that place a record (pass 0, copy_inactive) note
                              slot_of_id[id] -- a scattered 4-B store each, hidden in the stream
                              kernel: what the write-back goes by, in a step or on demand; 0: a
                              decomposed store, which keeps id_out[slot] instead */
  unsigned* order;         /* nparticles: record indices sorted by tile (pass 0: into rec_in,
                              the dead last; later passes: the migrants, into rec_out) */
  unsigned* tile_count;    /* nsort + 2: histogram of the counting sort (zero between uses) */
  unsigned* tile_offset;   /* nsort + 2: first sorted position of each bucket */
  unsigned* tile_cursor;   /* nsort + 2: next free position of each bucket during placement */
  uint4* chunks;           /* max_chunks: {begin, end, tile, windowed} into order[] */
  unsigned* collide_queue; /* nparticles: ids suspended at their first collision */
  /* one bit per particle id: handed to the collision stage in this step.  Set by the kernel
   * that builds the collision queue when the write-back is split (mark_suspended): the pass over
   * the ids leaves those alone -- the collision stage exports them itself -- and can therefore
   * run BESIDE the collision stage, on a stream of lowest priority. */
  unsigned* susp_ids;
  int mark_suspended;
  SuspendExtra* susp;      /* nparticles: side store of the collision stage's time slicing */
  double* susp_track;      /* nparticles, only with the scalar-flux tally (else null) */
  StealWork* steal;        /* the collision stage's rings and CU lists (neutral_kernels.hip) */
  /* The stream kernel's tile queues (neutral_tiled.hip, "asynchronous tile queue"): per tile an
   * append-only log of record slots whose histories left the tally window they were streaming
   * under with far to go and have reached this tile.  Producers reserve places with an atomic add
   * on queue_tail and store the slot (kQueueEmpty until then); workgroups claim ranges with a
   * compare-and-swap on queue_head and stream them under a window centred on the tile -- inside
   * the SAME launch: no sort, no further pass.  A tile that receives more than queue_capacity
   * in one launch overflows into the pass mechanism (kRecMigrate, sorted by the next pass).
   * null: no queues, every migrant waits for the next pass. */
  unsigned* queue_entries; /* ntiles * queue_capacity */
  unsigned* queue_tail;    /* ntiles: places reserved in this launch (may exceed the capacity) */
  unsigned* queue_head;    /* ntiles: places claimed by workgroups */
  unsigned queue_capacity;
  /* finer bucketed index for the collision stage (identical tables only; null: none) */
  const unsigned short* fine_index;
  int fine_index_n;
  long long fine_index_base;
  int fine_index_shift;
  int* edges_computed;     /* [device] 1: SolveArgs::edge_dx / edge_dy reproduce both edge arrays */
  unsigned char* tile_uniform; /* ntiles: 1 when every cell of the tile's window and of the ring
                                  around it holds one density (recomputed every step) */
  unsigned* ctrl;          /* 8 words: chunk head, #chunks, queue length, #active, #migrants,
                              passes used */
  int chunk_particles;     /* particles one workgroup takes at a time */
  int refill_min;          /* stream kernel: empty lanes of a wave that trigger a refill */
  int stream_repeat;       /* ... facet crossings of a wave per STREAM pass (scheduling only) */
  int pass;                /* 0: every live record starts its history; > 0: migrants resume */
  int allow_migrate;       /* 0 on the last permitted pass: finish with global atomics */
  double cells_per_x;      /* nx / mesh width, ny / mesh height: for the estimate of how */
  double cells_per_y;      /* many facets a history still has to cross */
  int tile_shift;          /* log2 of the tile edge in cells: 4 (16 cells) .. 7 (128) */
  int window_min_particles; /* a chunk with fewer particles tallies straight to HBM */
  int tiles_x;
  int tiles_y;
  int ntiles;
  int reach_classes;       /* 1, or 4: records are sorted by (tile, reach class) -- sparse
                              problems, neutral_history.h: reach_class */
  int nsort;               /* buckets of the counting sort: ntiles * reach_classes (+ the dead) */
  int max_chunks;
};

/* What the launches of a particle store are tuned by: constants of the kernels that tests and
 * A/B runs override from the environment, and the device's CU count.  Read ONCE per store (when
 * its records are imported), not per launch: three getenv and two runtime queries per collision
 * stage were test plumbing in the hot launch path. */
struct LaunchTuning {
  int steal_min;          /* NEUTRAL_STEAL_MIN (default kStealMin) */
  int share_weight;       /* NEUTRAL_SHARE_WEIGHT (default kOldestWeight) */
  int weighted_share_min; /* NEUTRAL_WEIGHTED_SHARE_MIN (default kWeightedShareMin) */
  int steal_delay;        /* NEUTRAL_STEAL_DELAY (default 0) */
  int max_blocks;         /* NEUTRAL_K2_MAX_BLOCKS (default 0: no cap) */
  int compute_units;
};
LaunchTuning launch_tuning_from_env();

/* spatial domain decomposition: px x py ranks, uniform blocks of bx x by cells (the
 * last ones may be smaller); rank r owns block (r % px, r / px) */
struct DomainGrid {
  int px, py;
  int bx, by;
};

/* what the host enqueues of a timestep of the tiled pipeline in one go */
struct TiledPlan {
  int stream_passes; /* stream passes to enqueue back to back (steady state: what the
                        last step needed plus one) */
  int blocks_per_cu; /* collision stage: workgroups per CU (0: as many as fit; -1: chosen by
                        the kernel from the queue length) */
};

enum Variant {
  kVariantOverParticle = 0, /* K1: one lane owns one history start to finish */
  kVariantEventSorted = 1,  /* K2: lanes re-grouped by next event */
  kVariantTiled = 2,        /* K3: tile-sorted streaming with an LDS tally window, then K2 */
};

hipError_t launch_inject(const InjectArgs& a, hipStream_t stream);
/* decomposed mesh: every rank looks at all a.nparticles candidates (positions in the
 * GLOBAL source box given by a.left_off ...) and keeps those that fall into its block
 * of the mesh (a.edgex / a.edgey are the block's edges); keys[slot] = global id,
 * *count = particles kept */
hipError_t launch_inject_filtered(const InjectArgs& a, unsigned* keys, unsigned* count,
                                  hipStream_t stream);
/* The energy-group flux spectrum over a box of cells (neutral_hip.h:
 * neutral_hip_set_spectrum_tally), as the kernels see it.  The box is in global cells. */
constexpr int kSpectrumMaxGroups = 64;
struct SpectrumParams {
  double* buffer; /* the step's 2 * ngroups values: track length by group, then collision */
  int ngroups;    /* (0: not kept) */
  int x0, y0;              /* the box: x0 <= cellx < x0 + width, y0 <= celly < y0 + height */
  unsigned width, height;
  double edges[kSpectrumMaxGroups + 1]; /* group g: edges[g] <= E < edges[g + 1] */
};
/* The net current per cell (neutral_hip.h: neutral_hip_set_current_tally), as the kernels see
 * it: the two meshes of this step's contributions, Jx and Jy (nx * ny doubles each; null: not
 * kept), and the pending x and y sums of the histories the collision stage's time slicing sets
 * aside (indexed like TiledArgs::susp_track: susp[2 * pid], susp[2 * pid + 1]; null outside the
 * tiled pipeline). */
struct CurrentParams {
  double* jx;
  double* jy;
  double* susp;
};
/* The in-step weight window (neutral_hip.h: neutral_hip_set_window_roulette), as the collision
 * kernels see it: the caller's mesh of lower bounds (null: off), max(ngroups, 1) meshes of
 * cny rows of cnx bins back to back; the transport mesh it was set for (global cells: a cell
 * outside it has no window, whatever else holds); the blocks' divisors (blocks == 0: the bins
 * are the cells) and the group edges (ngroups == 0: one mesh, no energy read). */
struct WindowRouletteParams {
  const double* lower;
  double survival_ratio;
  int nx, ny;
  int cnx, cny;
  int blocks;
  int ngroups;
  BlockDivisor by_x, by_y;
  double edges[kSpectrumMaxGroups + 1];
};
/* The leakage tally (neutral_hip.h: neutral_hip_set_leakage_tally), as the kernels that score the
 * outflow see it: the step's buffer of 2 * 4 * (ngroups + 1) * ncosines doubles -- the weights
 * times 1/N, then the counts; bin (side * (ngroups + 1) + group) * ncosines + cosine -- which the
 * ABI adds to the caller's array after the step (null: off), and the ABI's device copy of the
 * ngroups + 1 group edges (null with ngroups == 0): read by the lanes that leave, in the branch
 * that lets them, so the 65 doubles are no part of a kernel argument. */
constexpr int kLeakageMaxCosines = 64;
struct LeakageParams {
  double* buffer;
  const double* edges;
  int ngroups;
  int ncosines;
};
/* The escape bank (neutral_hip.h: neutral_hip_set_escape_bank), as the kernels that score the
 * outflow see it: the caller's records (null: off), the library's cursor on the device and the
 * capacity.  Read by the lanes that leave, in the branch that lets them. */
struct alignas(16) EscapeRecord { /* NeutralHipEscapeRecord, 64 bytes: four 16-byte words */
  double x, y;
  double omega_x, omega_y;
  double energy, weight;
  double time_left;
  unsigned slot, side;
};
static_assert(sizeof(EscapeRecord) == 64, "an escape record is four 16-byte words");
struct BankParams {
  EscapeRecord* records;
  unsigned long long* cursor;
  unsigned long long capacity;
};
/* Periodic axes (neutral_hip.h: neutral_hip_set_periodic_axes), as the kernels that score the
 * outflow see them: bit 0 -- x, west <-> east; bit 1 -- y, south <-> north; and
 * W = fl(edgex[global_nx] - edgex[0]), H likewise: what a wrap adds to or takes off a position.
 * `edges`: where the mesh's first and last edge of each axis lie on the device (x first, x last,
 * y first, y last) -- the kernel that stores the options works W and H out from them, one IEEE
 * subtraction each, on the stream of the launches that read them: no copy to the host and no wait.
 * Null (a rank that owns a block of the mesh and holds its own edges only): width and height are
 * the host's. */
struct PeriodicParams {
  unsigned axes;
  unsigned reserved;
  double width;
  double height;
  const double* edges[4];
};
/* The optional scoring of a step (neutral_hip.h), everything off as it stands here.  Each part
 * that is on is a compile-time property of the history kernels (Score below): the default
 * instantiations carry no trace of any. */
struct StepOptions {
  /* collision tallies: the step's buffer of 2 * nx * ny doubles -- the collisions, then the
   * absorbed weight -- which the ABI adds to the caller's meshes after the step */
  double* collision_tallies = nullptr;
  /* Russian roulette: the weight cutoff w_c and the survival weight w_s (0, 0: off).  The
   * kernels add what roulette did to the launch's StepCounters. */
  double roulette_cutoff = 0.0;
  double roulette_survival = 0.0;
  SpectrumParams spectrum = {}; /* (the kernels add their scores, times 1/N, to its buffer) */
  /* (with the current, SolveArgs::flux_tally must be a mesh -- the caller's, or one nobody
   * reads: scores_instantiated) */
  CurrentParams current = {nullptr, nullptr, nullptr};
  /* outflow tally (neutral_hip.h: neutral_hip_set_outflow_tally): the step's buffer of
   * 4 * nx * ny doubles -- the weight that left each cell through its west, east, south and
   * north side -- which the ABI adds to the caller's meshes after the step (null: not kept;
   * with it, SolveArgs::flux_tally must be a mesh, like with the current). */
  double* outflow = nullptr;
  /* the in-step weight window: roulette with the cutoff looked up per bin (never together with
   * roulette_cutoff > 0).  (Last: the fields above keep their offsets in the kernels' device
   * variable, and the kernels that read them their code.) */
  WindowRouletteParams window = {};
  /* vacuum sides (neutral_hip.h: neutral_hip_set_vacuum_sides): bit s set -- a history that would
   * reflect through outer side s (the outflow's numbering) escapes instead.  Read by the
   * instantiations that score the outflow, in the branch that reflects; with a bit set `outflow`
   * is a buffer even when the caller keeps no outflow tally.  (Last, for the reason above.) */
  unsigned vacuum_sides = 0;
  /* the leakage tally, scored where a history escapes.  (Last, for the reason above; not a Score:
   * it rides the outflow's instantiations like the vacuum sides it depends on.) */
  LeakageParams leakage = {};
  /* the escape bank, written where a history escapes.  (Last, like the leakage tally and for its
   * reasons.) */
  BankParams bank = {};
  /* periodic axes: a history that would reflect through a side of such an axis goes on from the
   * opposite side instead.  Read where the vacuum sides are, by the same instantiations; with an
   * axis set `outflow` is a buffer like under a vacuum side.  (Last, like everything above.) */
  PeriodicParams periodic = {};
};
/* ... and as the kernels' template argument: the sum of what is on */
enum Score : unsigned {
  kScoreCollisions = 1,
  kScoreRoulette = 2,
  kScoreSpectrum = 4,
  kScoreCurrent = 8,
  kScoreOutflow = 16,
  kScoreWindowRoulette = 32, /* (the second kind of roulette: instantiated without kScoreRoulette only) */
};
constexpr int kScoreBits = 6;
/* (what the stream kernel, which never collides, scores) */
constexpr unsigned kScoresOfStreaming = kScoreSpectrum | kScoreCurrent | kScoreOutflow;
constexpr int kStreamScoreBits = 5; /* (they lie in the low five: its launcher chooses among those) */
static_assert(kScoresOfStreaming < (1u << kStreamScoreBits), "the stream kernel's scores fit its launcher's bits");
inline unsigned scores_of(const StepOptions& o) {
  return (o.collision_tallies ? kScoreCollisions : 0u) | (o.roulette_cutoff > 0.0 ? kScoreRoulette : 0u) |
         (o.spectrum.ngroups > 0 ? kScoreSpectrum : 0u) | (o.current.jx ? kScoreCurrent : 0u) |
         (o.outflow ? kScoreOutflow : 0u) | (o.window.lower ? kScoreWindowRoulette : 0u);
}
/* the current and the outflow are instantiated with the scalar flux's code only; the two roulettes
 * exclude each other (neutral_hip.h), so no kernel is built for both */
constexpr bool scores_instantiated(bool flux, unsigned scores) {
  return (flux || !(scores & (kScoreCurrent | kScoreOutflow))) &&
         (scores & (kScoreRoulette | kScoreWindowRoulette)) != (kScoreRoulette | kScoreWindowRoulette);
}
/* The options of the launches that follow on `stream`, into a device variable of each
 * translation unit that scores them (neutral_step_options.h; nothing is enqueued when all are
 * off: no kernel then reads it).  They are not SolveArgs fields: a longer SolveArgs moves the
 * TiledArgs behind it in the stream kernel's arguments, and that alone changed the spills of
 * five stream kernel instantiations.  The launchers are given the same options: they choose the
 * instantiation and size its LDS by them. */
hipError_t set_step_options(const StepOptions& o, hipStream_t stream);
hipError_t set_step_options_tiled(const StepOptions& o, hipStream_t stream); /* (set_step_options') */
hipError_t launch_solve(const SolveArgs& a, const StepOptions& o, int variant, hipStream_t stream);
/* The in-step window's mesh as it is set (neutral_hip_set_window_roulette): the head of the
 * workspace says how many of the n entries are negative or not finite. */
struct MeshCheckHeader {
  unsigned long long bad;
};
hipError_t launch_window_mesh_check(const double* lower, long long n, void* workspace, hipStream_t stream);
/* The host's cached view of the two cs tables, re-checked on the device every step:
 * out[0] = 1 unless hash(scatter keys) == expect_hash_s, hash(absorb keys) ==
 * expect_hash_a and (tables element-wise identical) == expect_same; out[1], out[2] =
 * the two hashes, out[3] = the identity flag (all four words are written). */
/* out[0] |= 1 when a value lies outside [2^-100, 2^100] (zero, negative, inf, NaN too) */
hipError_t launch_unphysical_values(const double* v, long long n, unsigned long long* out,
                                    hipStream_t stream);
/* out: 16 words, the first 8 -- [0] the abort flag of the step's history kernels = [6] | [7]; [1..3]
 * hashes and identity; [4] a key or value lies outside [2^-100, 2^100]; [5] (written by
 * launch_unphysical_values before this kernel) a density does; [6] the expected hashes /
 * identity do not match; [7] fast_arithmetic was launched and [4] or [5] is set; [8..12]
 * the kernel's own accumulators (zero between launches) */
hipError_t launch_tables_check(const double* ks, const double* vs, int ns, const double* ka,
                               const double* va, int na, unsigned long long expect_hash_s,
                               unsigned long long expect_hash_a, int expect_same,
                               int fast_arithmetic, unsigned long long* out4,
                               hipStream_t stream);


/* tiled pipeline: sort by tile, stream with the LDS tally window, then K2 */
size_t tiled_lds_bytes(const SolveArgs& a, const StepOptions& o, const TiledArgs& t);
/* SoA store <-> record store (ids 0..n-1 in order on import; scatter by id on export) */
hipError_t launch_import_records(const ParticleView& p, ParticleRec* rec, unsigned* info,
                                 unsigned* slot_of_id, unsigned* ids, int tiles_x, int tile_shift,
                                 int x_off, int y_off, int n, hipStream_t stream);
/* carried_in[slot].micro for every live record of t.rec_in, by plain bisection of the scatter table (no
 * index: independent of the cached view) -- after an import, after the table view was rebuilt */
hipError_t launch_refresh_micro(const SolveArgs& a, const TiledArgs& t, hipStream_t stream);
/* does this step's stream kernel start histories from the carried values? */
bool tiled_uses_carried(const SolveArgs& a, const TiledArgs& t);
/* slot_of_id: where each id's record is (TiledArgs::slot_of_id) */
/* Records in slots from a boundary on belong to particles whose final state the arrays hold
 * already and are left alone (the random access to them is what the pass is bound by):
 * first_inactive [device] -- the first slot of the particles that were dead when the step
 * began, given when the arrays were current then -- or, when that is null, final_from [host
 * value]: the graveyard's first slot at the time the arrays were last current (0xFFFFFFFF:
 * every record is written). */
hipError_t launch_export_records(const ParticleRec* rec, const unsigned* slot_of_id,
                                 const ParticleView& p, int n, hipStream_t stream,
                                 const int* abort_flag = nullptr,
                                 const unsigned* first_inactive = nullptr,
                                 unsigned final_from = 0xFFFFFFFFu,
                                 const unsigned* skip_ids = nullptr, int max_blocks = 0,
                                 bool partial_ok = false);
/* the write-back split in two (see TiledArgs::susp_ids): what launch_solve_tiled enqueues on a
 * stream of its own, beside the collision stage, when `on` */
struct SplitExport {
  bool on;
  hipStream_t side;      /* (low priority: it gets the CUs the collision stage's waves leave) */
  hipEvent_t done;       /* recorded on `side` after the pass */
  ParticleView p;
  int skip_long_dead;
};
const unsigned* tiled_first_inactive(const TiledArgs& t);
/* spatial domain decomposition (neutral_tiled.hip, section 2b): emigrants of this
 * step's records (t.rec_out) counted and packed by destination rank, arrivals appended
 * behind the first_slot records, holes closed at the end of the step (t.rec_out ->
 * t.rec_in; *cursor = records kept), and the slot-for-slot exchange with the SoA store */
hipError_t launch_emigrant_count(const TiledArgs& t, int n, const DomainGrid& d, unsigned* counts,
                                 hipStream_t stream);
hipError_t launch_emigrant_pack(const TiledArgs& t, int n, const DomainGrid& d,
                                const unsigned* offset, unsigned* cursor, ParticleRec* send,
                                unsigned* free_slots, unsigned* nfree, hipStream_t stream);
/* (the first `reuse` arrivals take the last entries of the free list of nfree slots) */
hipError_t launch_immigrant_append(const TiledArgs& t, const ParticleRec* recv, int nrecv,
                                   int first_slot, int x_off, int y_off,
                                   const unsigned* free_slots, int nfree, int reuse,
                                   hipStream_t stream);
hipError_t launch_compact_records(const TiledArgs& t, int n, unsigned* cursor, hipStream_t stream);
hipError_t launch_import_by_slot(const ParticleView& p, const unsigned* keys, const TiledArgs& t,
                                 int x_off, int y_off, int n, hipStream_t stream);
hipError_t launch_export_by_slot(const ParticleRec* rec, const ParticleView& p, unsigned* keys,
                                 int n, hipStream_t stream);
/* tile edge (log2 cells) and window threshold for a problem; tiles and chunk capacity */
int tiled_tile_shift(int nx, int ny, int nparticles, bool with_flux);
int tiled_window_min_particles(int tile_shift);
void tiled_geometry(int nx, int ny, int nparticles, int tile_shift, int* tiles_x, int* tiles_y,
                    int* max_chunks);
/* Enqueues plan.stream_passes stream passes starting with pass number first_pass, the
 * collision queue and the collision stage; nothing here waits for the device.
 * a.counters must point at TWO StepCounters records: [0] streaming kernel, [1]
 * collision kernel.  The optional events are recorded after the first sort, after
 * the last enqueued streaming pass and after the collision queue is built.  The
 * caller reads t.ctrl (migrants left over, passes used, queue length) with the
 * step's counters and calls again with first_pass = *passes_enqueued while migrants
 * are left (histories suspended by the later passes get a collision stage of their
 * own; the earlier ones are marked done).  This step's records are t.rec_out /
 * t.info_out: the caller swaps in/out when the step is complete. */
hipError_t launch_solve_tiled(const SolveArgs& a, const StepOptions& o, TiledArgs& t, hipStream_t stream,
                              const TiledPlan& plan, int first_pass, hipEvent_t after_sort,
                              hipEvent_t after_stream, hipEvent_t after_collect,
                              int* passes_enqueued, const SplitExport* split = nullptr);
hipError_t launch_split_export(const SolveArgs& a, const TiledArgs& t, const SplitExport& split,
                               hipEvent_t after_collect);


/* builds start[0..nbuckets] of the bucketed index for `keys` (neutral_device.h) */
hipError_t launch_build_cs_index(const double* keys, int n, int shift, long long base,
                                 int nbuckets, unsigned short* start, hipStream_t stream);

/* unit probes of the device building blocks (all pointers [device]) */
hipError_t launch_probe_threefry(const uint64_t* in, uint64_t* out, double* rn, int n,
                                 hipStream_t stream);
struct CsIndex;
hipError_t launch_probe_cs(const double* keys, const double* values, int nentries,
                           const double* energy, double* value, int* index, int n,
                           const CsIndex& ix, hipStream_t stream);
hipError_t launch_probe_facet(const double* in, double* dist, int* x_facet, int n,
                              hipStream_t stream);
hipError_t launch_probe_division(const double* in, double* out, int* plain, int n,
                                 hipStream_t stream);
hipError_t launch_probe_log(const double* in, double* out, int n, hipStream_t stream);
hipError_t launch_probe_scatter(const double* in, double* out, int n, hipStream_t stream);
hipError_t launch_probe_policy_quotient(const double* in, double* out, int n, hipStream_t stream);
hipError_t launch_probe_policy_root(const double* in, double* out, int n, hipStream_t stream);

/* ---- between two timesteps: comb, source, window, and the census tally with the bounds made
 * from it (neutral_comb.hip; include/neutral_hip.h) ----
 * The first three share their scans, all five one allocation and one host protocol
 * (neutral_abi_store.hip: run_census_op).  The scans work on tiles of kCombTile elements, one workgroup each: a store of up
 * to one tile is scanned by one workgroup, up to kCombTile^2 through one level of tile sums, beyond
 * that through two (kCombTile^3 = 2^33 covers every int count).
 * The workspace is one allocation that every call grows to what it asks for: a header of 256 bytes
 * at its head (each operation's own struct, below: what its kernels tell each other and the host)
 * and behind it the operation's own rooms and no others (neutral_comb.hip: the *Rooms structs).
 * Every launch_* below enqueues everything on `stream` without a wait in between; its header is
 * complete when the stream has drained. */
constexpr int kCombBlock = 256;
constexpr int kCombItems = 8; /* consecutive elements per lane */
constexpr int kCombTile = kCombBlock * kCombItems;
size_t comb_workspace_bytes(int n);   /* n doubles, two arrays of n unsigned, the scans' tile sums */
size_t window_workspace_bytes(int n); /* the same and one byte per slot */
size_t source_workspace_bytes(int n); /* n unsigned and the tile sums of a u32 scan */

/* ---- census weight comb (neutral_hip_comb_particles) ---- */
struct CombHeader {
  double offset;       /* v */
  double weight;       /* W, the last prefix sum */
  double weight_each;  /* W / n */
  unsigned long long live;
  unsigned long long bad;     /* != 0: a live weight is negative or not finite */
  unsigned long long sources; /* particles that received a tooth */
  unsigned long long max_copies;
  unsigned long long go;      /* 1: the store is rewritten; 0: every later kernel returns at entry */
};
/* Scan and tooth counts, the decision (CombHeader::go), the expansion to src[], the gather field by
 * field through the n doubles, the new weight and dead arrays.  The two unsigned arrays: teeth
 * below each prefix sum; the source of each slot. */
hipError_t launch_comb(const ParticleView& p, int n, uint64_t pkey, uint64_t seed, void* workspace,
                       hipStream_t stream);

/* ---- fixed source (neutral_hip_source_particles) ---- */
struct SourceHeader {
  unsigned long long dead;    /* slots with dead != 0 going in */
  unsigned long long emitted; /* slots refilled: min(count, dead) */
};
/* The ranks of the dead slots of a.p (an inclusive u32 sum-scan of the dead flags) and the refill
 * of those of rank <= count with inject_slot(a, slot, seed, weight, plain_source(a)): the last scan pass writes the
 * slots in rank order (into its list of n unsigned) and a kernel of one lane per refilled slot
 * follows. */
hipError_t launch_source(const InjectArgs& a, int n, int count, double weight, uint64_t seed,
                         void* workspace, hipStream_t stream);

/* ---- described source (neutral_hip_source_described) ---- */
constexpr int kDescribedMaxComponents = 16;
constexpr int kDescribedMaxBins = 256;
/* a component and a bin as the fill reads them: the caller's, a component with the running sums
 * made on the host (left to right, one addition each) in place of its share.  The bins keep their
 * shares: two components may read one bin, each with a running sum of its own, which the fill
 * makes as it walks -- the same additions in the same order. */
struct DescribedComponent {
  double left, bottom, width, height;
  double theta0, theta_width;
  double cumulative; /* C_k: the shares of components 0 .. k */
  double bin_total;  /* S_k: the shares of all its bins */
  int bin_first, bin_count;
};
struct DescribedBin {
  double e_lo, e_hi, share;
};
struct DescribedTables {
  DescribedComponent components[kDescribedMaxComponents];
  DescribedBin bins[kDescribedMaxBins];
};
struct DescribedSourceHeader {
  SourceHeader base;
  unsigned long long by_component[kDescribedMaxComponents]; /* slots refilled out of each component */
};
size_t described_workspace_bytes(int n); /* the source's workspace and the two tables behind it */
/* launch_source's scan and list, then a fill of one lane per refilled slot that chooses component
 * and bin with counter 2 of the slot's stream and calls inject_slot with what they say.
 * *host_tables is copied into the workspace on `stream`: it stays the caller's until the stream has
 * drained.  a's own box and energy are not looked at. */
hipError_t launch_described_source(const InjectArgs& a, int n, int count, double weight, uint64_t seed,
                                   const DescribedTables* host_tables, int ncomponents, int nbins,
                                   void* workspace, hipStream_t stream);

/* ---- mesh source (neutral_hip_source_mesh) ---- */
/* the one spectrum of a mesh source as the fill reads it: the caller's bins with their shares (the
 * fill makes the running sums as it walks, as the described source's does) */
struct MeshSourceBins {
  DescribedBin bins[kDescribedMaxBins];
};
struct MeshSourceHeader {
  SourceHeader base;
  unsigned long long nonzero; /* K: cells with strength > 0 */
  unsigned long long bad;     /* != 0: a strength is negative or not finite */
  unsigned long long go;      /* 1: the fill runs; 0: it returns at entry */
  double total;               /* S: the last of the cumulative sums */
};
struct MeshSourceArgs {
  const double* strength; /* [device] local_ny rows of local_nx */
  double theta0, theta_width;
  double bin_total; /* the shares of all bins: the host's running sum */
  int nbins;
};
constexpr long long kMeshSourceMaxCells = 1ll << 30;
/* the source's workspace, and behind it the bins, the cumulative table of `cells` doubles, two arrays
 * of `cells` unsigned and the tile sums of a scan over the cells */
size_t mesh_source_workspace_bytes(int n, long long cells);
/* launch_source's scan and list; over the cells (a.local_nx * a.local_ny of them) a u32 rank scan of
 * strength > 0 and the f64 scan of the strengths, which stores C_c and c at the rank of every
 * non-zero cell; one thread's decision (MeshSourceHeader::go); a fill of one lane per refilled slot
 * that bisects the K cumulative sums with counter 2 of the slot's stream and calls inject_slot
 * with the cell's box and the cell itself.  *host_bins is copied into the workspace on `stream`: it
 * stays the caller's until the stream has drained.  a's own box and energy are not looked at. */
hipError_t launch_mesh_source(const InjectArgs& a, int n, int count, double weight, uint64_t seed,
                              const MeshSourceArgs& m, const MeshSourceBins* host_bins, void* workspace,
                              hipStream_t stream);

/* ---- bank source (neutral_hip_source_bank) ---- */
struct BankSourceHeader {
  SourceHeader base;
  unsigned long long first_bad; /* the lowest index into records[] of a record the call refuses (~0: none) */
  unsigned long long snapped;   /* coordinates moved onto a wall */
  double weight;                /* the sum of the weights written */
};
struct BankSourceArgs {
  const EscapeRecord* records; /* [device] */
  unsigned long long first;
  double weight_scale;
  double snap;
  double shift[8]; /* dx, dy for side 0 .. 3 */
};
size_t bank_source_workspace_bytes(int n); /* the fixed source's */
/* launch_source's scan and list; a pass of one lane per slot that would be refilled over its record
 * (slot of rank k: records[first + k]), which keeps the lowest bad index; a fill of as many lanes,
 * which returns at entry when there is one: four 16-byte loads of the record, the shift, the snap,
 * the cell by bisection of the edges, the eleven fields.  No random number is drawn.  a's box and
 * energy are not looked at. */
hipError_t launch_bank_source(const InjectArgs& a, int n, int count, const BankSourceArgs& b, void* workspace,
                              hipStream_t stream);

/* ---- census weight window (neutral_hip_window_particles) ---- */
struct WindowHeader {
  unsigned long long live, dead;       /* slots with dead == 0 / != 0 going in */
  unsigned long long killed, survived; /* roulette, of the live slots under their bound */
  unsigned long long above;            /* live slots over their upper bound with m >= 2 */
  unsigned long long split;            /* of those, the ones granted at least one copy */
  unsigned long long demand;           /* copies asked for: the sum of m - 1 */
  unsigned long long free_slots;       /* F: dead going in, or killed by this call's roulette */
  unsigned long long granted;          /* min(demand, F): one lane of the fill each */
  unsigned long long bad;              /* != 0: a live slot the call refuses (neutral_hip.h) */
  unsigned long long go;               /* 1: the writing kernels run; 0: they return at entry */
  double lost, gained;                 /* roulette: sum of w over the killed, of w_s - w over the survivors */
};
struct WindowArgs {
  const double* lower; /* [device] ny * nx */
  int nx, ny;
  double upper_ratio, survival_ratio;
  int max_split;
  uint64_t pid_base, seed;
};
/* The classification (the only pass that reads the store's 20 bytes per slot, and the roulette
 * draws; its verdict is the byte per slot), the ranks of the free slots, the decision
 * (WindowHeader::go), the 64-bit scan of the demands with the heads of owner[], its running
 * maximum, roulette's stores, the copies.  The n doubles: the new weight of every source; the two
 * unsigned arrays: the free slots in ascending order, the owner of every granted request. */
hipError_t launch_window(const ParticleView& p, int n, const WindowArgs& a, void* workspace,
                         hipStream_t stream);

/* ---- energy groups for the window and the census (neutral_hip_window_particles_groups,
 * neutral_hip_census_tally_groups) ----
 * Both passes over the store have a grouped form, a compile-time parameter of their kernels: a live
 * lane loads its energy beside the 20 bytes it reads anyway and finds its group by a bisection of
 * the G + 1 edges, which every workgroup stages in LDS once (at most 520 bytes; seven probes).
 * Bin b = (g * ny + celly) * nx + cellx: G meshes back to back, a mesh of nx by G * ny to
 * everything that comes after the pass.  A live slot in no group is checked like the others,
 * counted, and otherwise left out.  The plain instantiations carry no trace of any of it. */
struct GroupWindowHeader {
  WindowHeader window;
  unsigned long long outside; /* live slots in no group */
};
size_t window_groups_workspace_bytes(int n); /* the window's workspace and the edges behind it */
/* launch_window with a.lower holding ngroups * a.ny * a.nx bounds.  host_edges[0 .. ngroups] is
 * copied into the workspace on `stream`: it stays the caller's until the stream has drained. */
hipError_t launch_window_groups(const ParticleView& p, int n, const WindowArgs& a, int ngroups,
                                const double* host_edges, void* workspace, hipStream_t stream);

/* ---- census tally (neutral_hip_census_tally) and window bounds (neutral_hip_window_bounds) ----
 * Both work on meshes, not on slots: their workspace is sized by the cells -- a header of 256
 * bytes, the census's own mesh of 2 * cells doubles and one double more (the refusal flag: with
 * several ranks the mesh and the flag are summed over them in one all-reduce), and the tile sums of
 * four reductions over the cells (comb_reduce_tiles_kernel, level upon level down to one value). */
size_t census_workspace_bytes(int nx, int ny);
constexpr int kCensusMaxBlocks = 2048; /* the pass over the store is grid-strided: eight workgroups per CU */
struct CensusHeader {
  unsigned long long live, dead;    /* this rank's slots with dead == 0 / != 0 */
  unsigned long long bad;           /* != 0: this rank saw a live slot the call refuses */
  unsigned long long occupied;      /* cells with count > 0 (over the ranks) */
  unsigned long long max_count;
  unsigned long long go;            /* 1: out holds the meshes; 0: out holds zeros */
  double weight, max_cell_weight;
};
/* The first half: header and mesh zeroed, the one pass over the store (20 bytes per slot, two
 * no-return f64 atomics per live lane), the flag behind the mesh.  -> census_mesh(workspace) holds
 * census_mesh_doubles(nx, ny) values to sum over the ranks. */
hipError_t launch_census_score(const ParticleView& p, int n, int nx, int ny, void* workspace,
                               hipStream_t stream);
double* census_mesh(void* workspace);
size_t census_mesh_doubles(int nx, int ny);
/* The second half, on the (summed) mesh: occupied cells, largest count, weight and largest weight
 * by four reductions, the decision (CensusHeader::go), and out[0 .. 2 * cells): the counts, then the
 * weights -- or zeros where the flag is up. */
hipError_t launch_census_finish(int nx, int ny, double* out, void* workspace, hipStream_t stream);
/* The grouped census is launch_census_score_groups, the all-reduce of census_mesh_doubles(nx,
 * ngroups * ny) values and launch_census_finish(nx, ngroups * ny, ...): its workspace is that mesh's
 * with the edges behind it, and its header has one counter more. */
struct GroupCensusHeader {
  CensusHeader census;
  unsigned long long outside; /* this rank's live slots in no group */
};
size_t census_groups_workspace_bytes(int nx, int ny, int ngroups);
hipError_t launch_census_score_groups(const ParticleView& p, int n, int nx, int ny, int ngroups,
                                      const double* host_edges, void* workspace, hipStream_t stream);

/* ---- blocks of cells for the census and the window (neutral_hip_census_tally_blocks,
 * neutral_hip_window_particles_blocks) ----
 * The bins lie on a coarse mesh of cnx by cny blocks, max(G, 1) of them back to back: a mesh of cnx
 * by max(G, 1) * cny to launch_census_finish and launch_bounds.  Both passes over the store take the
 * cell-to-block map as a second compile-time parameter beside the groups; the unit-cell
 * instantiations are the plain and grouped calls' kernels as they were.  ngroups 0: no groups.
 * Workspaces: census_groups_workspace_bytes(cnx, cny, max(ngroups, 1)) and
 * window_groups_workspace_bytes(n); the headers are the grouped calls', `outside` 0 without groups.
 * The census pass keeps its bins in LDS where they number at most min(lds_max_bins,
 * kCensusLdsBinsMax) -- 12 bytes a bin, workgroups as many as are resident on compute_units CUs,
 * each flushing its non-empty bins with one global add per bin and mesh -- and is the two global
 * atomics per live lane above that; *privatised says which it was. */
struct BlockMesh {
  int block_x, block_y;
  int cnx, cny; /* ceil(nx / block_x), ceil(ny / block_y) */
  static BlockMesh of(int nx, int ny, int block_x, int block_y) {
    return BlockMesh{block_x, block_y, (int)(((long long)nx + block_x - 1) / block_x),
                     (int)(((long long)ny + block_y - 1) / block_y)};
  }
};
constexpr int kCensusLdsBinsMax = 4096; /* 48 KB of LDS: three workgroups per CU */
constexpr int kCensusLdsBins = 4096;    /* the cap as shipped (profiles/block_window/README.md);
                                           NEUTRAL_CENSUS_LDS_BINS overrides it per call, 0: never */
hipError_t launch_census_score_blocks(const ParticleView& p, int n, int nx, int ny, const BlockMesh& b,
                                      int ngroups, const double* host_edges, int lds_max_bins,
                                      int compute_units, void* workspace, hipStream_t stream,
                                      bool* privatised);
/* launch_window with a.lower holding max(ngroups, 1) * b.cny * b.cnx bounds; a.nx, a.ny stay the
 * transport mesh's, which the cells are checked against */
hipError_t launch_window_blocks(const ParticleView& p, int n, const WindowArgs& a, const BlockMesh& b,
                                int ngroups, const double* host_edges, void* workspace, hipStream_t stream);

struct BoundsHeader {
  unsigned long long eligible;   /* K */
  unsigned long long floored;    /* eligible cells with fl(W_c / M) < floor_ratio */
  unsigned long long bad;        /* != 0: a census entry is negative or not finite */
  unsigned long long go;         /* 1: lower_out is written; 0: it stays as it is */
  double max_cell_weight;        /* M over the eligible cells */
  double peak;                   /* the bound of the cell that holds M */
};
struct BoundsArgs {
  const double* census; /* [device] 2 * ny * nx: counts, then weights */
  int nx, ny;
  double target_population, upper_ratio, floor_ratio;
  int min_count;
};
/* K, M and the bad-entry flag by three reductions, one thread's decision and peak
 * (BoundsHeader::go), one lane per cell for lower_out. */
hipError_t launch_bounds(const BoundsArgs& a, double* lower_out, void* workspace, hipStream_t stream);

/* ---- batch statistics (neutral_hip_batch_fold, neutral_hip_batch_statistics) ----
 * On any array of len doubles: no store, no mesh.  The workspace is a header of 256 bytes and the
 * tile sums of six reductions over the entries. */
size_t batch_workspace_bytes(size_t len);
struct BatchHeader {
  unsigned long long nonzero;                   /* fold: entries of x that are not 0.0 */
  unsigned long long scored, within10, within5; /* statistics: entries with a mean != 0, and their relerr */
  unsigned long long bad;                       /* != 0: an entry the call refuses */
  unsigned long long go;                        /* 1: the writing pass runs; 0: it returns at entry */
  double sum;                                   /* fold: of x; statistics: of estimate_out */
  double max_relerr, relerr_sum, mean_relerr;
};
/* The check (a reduction), sum and count, the decision (BatchHeader::go), Welford's update of the
 * 2 * len moments with batch number k. */
hipError_t launch_batch_fold(const double* x, size_t len, int k, double* moments, void* workspace,
                             hipStream_t stream);
/* The check, the decision, one lane per entry for estimate_out and relerr_out, six reductions over
 * what was written. */
hipError_t launch_batch_statistics(const double* moments, size_t len, int nbatches, double scale,
                                   double* estimate_out, double* relerr_out, void* workspace,
                                   hipStream_t stream);

}  // namespace neutral
#endif
