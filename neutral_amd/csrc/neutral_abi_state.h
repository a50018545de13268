/*
 * neutral_abi_state.h -- what the translation units of the C ABI share: the library's state
 * (one per process: a process drives one GPU), the types it is made of, and the helpers of one
 * unit that another calls.
 *   neutral_abi.hip           the three functions of the reference's neutral_interface.h
 *   neutral_abi_store.hip     particle stores, the tiled workspace and its record mirror, the
 *                             cached view of the cs tables, the HBM allocation / copy hooks,
 *                             settings, probes
 *   neutral_abi_exchange.hip  what crosses to the host or to other ranks at the end of a batch
 *                             of launches: the published results, the tally exchange, the
 *                             particle exchange of a decomposed mesh
 */
#ifndef NEUTRAL_AMD_ABI_STATE_H
#define NEUTRAL_AMD_ABI_STATE_H

#include "../../include/neutral_hip.h"

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "neutral_comm.h"
#include "neutral_kernels.h"

extern "C" {
#include "../host/comms.h"
}

extern "C" {
/* host layer (neutral_amd/host/host.c), linked into this library */
int get_key_value_parameter(const char* specifier, const char* filename, char* keys,
                            double* values, int* nkeys);
int within_tolerance(const double expected, const double result, const double tolerance);
}

#define NEUTRAL_ABI_VERSION 12 /* 12: set_collision_tallies; 11: probe_policy_quotient, probe_policy_root, probe_scatter's last column; 10: probe_scatter; 9: NeutralHipStepStats grew weighted_waves, stream_clock_ghz, collide_clock_ghz; 8: NeutralHipStepStats grew steals_refused, stream_hops, stream_overflows; 7: NeutralHipStepStats grew steals; 6: set_arithmetic, NeutralHipStepStats grew checked_arithmetic, attempts, host_collectives, exchange_ranks; 5: NeutralHipStepStats grew export_ms; 2: probe_division, NeutralHipStepStats grew requeued + collide_passes; 3: probe_log;
                                 4: invalidate_particles, NeutralHipStepStats grew host_syncs, stream_passes_enqueued, tile_cells */
#define NEUTRAL_MAX_KEYS 40
#define NEUTRAL_MAX_STR_LEN 1024
#define NEUTRAL_VALIDATE_TOLERANCE 1.0e-3 /* neutral_data.h:27 */

#define HIP_CHECK(expr)                                                              \
  do {                                                                               \
    hipError_t err_ = (expr);                                                        \
    if (err_ != hipSuccess) {                                                        \
      fprintf(stderr, "libneutral_hip: %s failed: %s\n%s:%d\n", #expr,               \
              hipGetErrorString(err_), __FILE__, __LINE__);                          \
      exit(EXIT_FAILURE);                                                            \
    }                                                                                \
  } while (0)

#include "neutral_device.h"


namespace neutral_abi {


constexpr int kMaxIndexBuckets = 16384; /* u16 entries: 32 KB of LDS at most */
/* The collision stage has the LDS to itself (three workgroups per CU): when both
 * tables are the same data it searches through an index of twice the resolution
 * (512 buckets per binade, 17 004 entries = 34 KB for the shipped table: the
 * window to bisect shrinks from 4.5 to 2.8 keys on average, from 28 to 16 at most) */
constexpr int kMaxFineIndexBuckets = 24576;

/* What the library derives from the two cs tables and keeps from step to step: are
 * they the same data (one search per energy), and the bucketed indexes over their
 * keys.  Keyed by the table pointers and sizes; the CONTENTS are re-checked on the
 * device every step (tables_check_kernel), so rewriting a table in place is noticed. */
struct TableView {
  bool valid = false;
  const double* keys_s = nullptr;
  const double* values_s = nullptr;
  int n_s = 0;
  const double* keys_a = nullptr;
  const double* values_a = nullptr;
  int n_a = 0;
  int variant = -1;
  unsigned long long hash_s = 0;
  unsigned long long hash_a = 0;
  int same = 0;
  neutral::CsIndex ix_s = {nullptr, 0, 0, 0};
  neutral::CsIndex ix_a = {nullptr, 0, 0, 0};
  neutral::CsIndex fine = {nullptr, 0, 0, 0};
};

struct StepResults {
  neutral::StepCounters counters[2];
  unsigned long long check[8];
  unsigned ctrl[16];
  unsigned long long words[20]; /* kStepWords */
  double roulette_weights[2]; /* several ranks: the step's weight lost and gained, all ranks */
  double escape[8];           /* ... and its escapes by side, then their weights (StepScalar) */
  double wrap[8];             /* ... and its wraps through periodic axes, likewise */
  unsigned long long bank_cursor; /* the escape bank's cursor, this rank's own (0 in a step that does not record) */
};

/* A device buffer grown on demand, and how many elements it was allocated for. */
template <class T>
struct Grown {
  T* d = nullptr;
  size_t capacity = 0;
};
/* Frees and reallocates `b` for `alloc` elements of `each` bytes (one at least) when `want` exceeds
 * its capacity, or when the caller has a reason of its own (`force`); -> whether it did. */
template <class T>
bool ensure_capacity(Grown<T>& b, size_t want, size_t alloc, size_t each = sizeof(T), bool force = false) {
  if (want <= b.capacity && !force) {
    return false;
  }
  if (b.d) HIP_CHECK(hipFree(b.d));
  HIP_CHECK(hipMalloc((void**)&b.d, each * (alloc ? alloc : 1)));
  b.capacity = alloc;
  return true;
}

/* A tally the kernels score per cell (nx * ny doubles per mesh) and the buffer a step's
 * contributions to it go through on their way to the caller: summed over the ranks that share
 * the mesh, added to the caller's mesh(es), cleared for what a further pass of the step adds. */
constexpr int kMaxMeshesPerTally = 4;
struct MeshTally {
  int meshes;       /* of the caller: 1, 2 (collisions, absorbed weight; Jx, Jy) or 4 (the outflow's
                       sides) back to back in the step buffer */
  int spare_meshes; /* behind them, meshes nobody reads, zeroed only when allocated: the current
                       and the outflow run the scalar flux's code, and a caller who keeps no
                       flux has it score into one */
  bool always_buffered; /* false: the kernels score straight into the caller's mesh unless
                           several ranks share it */
  /* (null: not kept; all or none.  The outflow's four are one caller buffer: [0] is what the
   * caller gave, the others follow from the mesh's size when a step begins) */
  double* caller[kMaxMeshesPerTally] = {nullptr, nullptr, nullptr, nullptr};
  Grown<double> step = {};  /* the buffer: capacity in cells per mesh */
  double* scored = nullptr; /* this step: step.d when its kernels score there, else null */
};
enum MeshTallyId : int { kTallyEnergy = 0, kTallyFlux, kTallyCollisions, kTallyCurrent, kTallyOutflow, kMeshTallies };

/* The step's f64 scalars, one block: what several ranks sum in one all-reduce beside the step
 * words -- the weight roulette lost and gained, the escapes through vacuum sides (four counts,
 * exact as doubles below 2^53, and the four sums of their weights), then the step's spectrum
 * (2 * ngroups). */
enum StepScalar : int {
  kScalarRouletteLost = 0,
  kScalarRouletteGained = 1,
  kScalarEscaped = 2,
  kScalarEscapeWeight = 6,
  kScalarWrapped = 10, /* (periodic axes: the wraps by the side left through, like the escapes) */
  kScalarWrapWeight = 14,
  kScalarSpectrum = 18,
  kStepScalars = kScalarSpectrum + 2 * neutral::kSpectrumMaxGroups,
};

/* The record mirror.  The tiled variant keeps the store it steps twice: the caller's eleven SoA
 * arrays, and the records in the tiled workspace (TiledArgs::rec_in / rec_out and what travels with
 * them).  This struct alone knows whose store the records mirror and which copy is current; nothing
 * outside its members writes that down.  The states:
 *   no owner                    the records mirror nothing; arrays current (the initial state)
 *   owner, records dropped      the arrays are the truth: the next tiled step of the store imports them
 *   owner, records current ...  the next tiled step of the store starts from the records, and
 *     ... arrays current          the arrays hold the same state (an eager step wrote it back)
 *     ... arrays stale            a write-back is pending (lazy export): whoever reads the arrays
 *                                 calls write_back() first
 * (Records dropped and arrays stale does not occur: whoever drops has written back first, or rewrites
 * the whole store.)  The operations, and between which states they move:
 *   adopt()             after write_back() and drop() for the previous owner: -> owner, records and
 *                       arrays current (the records were just imported from the arrays)
 *   rolled()            a step ended, records current -> arrays current (eager) or stale (lazy); the
 *                       planning hints of the next step (stream passes, the split write-back's share)
 *   write_back()        arrays stale -> arrays current, by one export and one wait; anywhere else it
 *                       launches nothing
 *   drop()              records current -> records dropped (the owner is kept; the hints start over)
 *   arrays_rewritten()  the owner's arrays were written to: -> records dropped; whole_store: a pending
 *                       write-back is discarded with them, the arrays are current by decree
 *   forget()            the owner is freed: -> no owner, pending state dies with it
 *   compacted(), holes_changed()                   a decomposed store's count and holes; no move
 *   carried_refreshed(), tables_changed()          TiledArgs::carried_in; no move */
struct RecordMirror {
  bool owns(const NeutralHipParticle* p) const { return rec_owner == (const void*)p->x; }
  /* does the next tiled step of p's n particles start from the records as they are? */
  bool mirrors(const NeutralHipParticle* p, int n) const { return rec_valid && owns(p) && rec_count == n; }
  bool arrays_current() const { return soa_valid; }
  bool carried_current() const { return carried_valid; }
  int planned_passes() const { return plan_passes; }
  double last_suspended_share() const { return suspended_share; }
  int holes() const { return free_count; }
  /* does [p, p + bytes) overlap one of the arrays of the store whose records are current? */
  bool overlaps(const void* p, size_t bytes) const;

  void write_back(); /* safe with any (or no) store in hand: the owner's arrays are remembered */
  void drop() {
    rec_valid = false;
    carried_valid = false; /* (TiledArgs::carried_in belongs to the records) */
    suspended_share = -1.0;
    free_count = 0; /* (slots emigrants left are holes of the records, not of the arrays) */
    plan_passes = 0;
  }
  void adopt(const NeutralHipParticle* p, const neutral::ParticleView& view, unsigned* keys /* decomposed, or null */,
             int count) {
    final_from = 0xFFFFFFFFu;
    rec_owner = (const void*)p->x;
    rec_owner_view = view;
    rec_owner_keys = keys;
    rec_count = count;
    rec_valid = true;
  }
  void arrays_rewritten(const NeutralHipParticle* p, bool whole_store) {
    if (owns(p)) {
      drop();
      soa_valid = soa_valid || whole_store;
    }
  }
  void forget(const NeutralHipParticle* p) {
    if (owns(p)) {
      rec_owner = nullptr;
      drop();
      soa_valid = true;
    }
  }
  /* stream_passes: what the step needed; by_id: not decomposed, and then whether the step kept the carried cross
   * sections, what share of its particles went to the collision stage, where its graveyard starts (sort_end) */
  void rolled(int stream_passes, bool lazy_export, bool by_id, bool carried_kept, double share, int graveyard) {
    plan_passes = stream_passes > 0 ? stream_passes : 1;
    soa_valid = !lazy_export; /* eager: exported by the step (or by its kernels) */
    if (by_id) {
      carried_valid = carried_valid && carried_kept; /* (a step that looked up and drew itself kept none) */
      suspended_share = share;
      if (soa_valid) final_from = (unsigned)graveyard; /* (arrays current: so is the graveyard in them) */
    }
  }
  void compacted(int kept) {
    free_count = 0; /* (the holes are closed: nothing to reuse next step) */
    rec_count = kept;
  }
  void holes_changed(int by) { free_count += by; } /* emigrants open them, arrivals fill them */
  void carried_refreshed() { carried_valid = true; }
  void tables_changed() { carried_valid = false; } /* (looked up in other tables) */

 private:
  const void* rec_owner = nullptr;           /* particles->x of the mirrored SoA store */
  neutral::ParticleView rec_owner_view = {}; /* its arrays, for the write-back */
  unsigned* rec_owner_keys = nullptr;        /* its keys[] when it is decomposed */
  int rec_count = 0;
  bool rec_valid = false;     /* records hold the current state */
  bool carried_valid = false; /* ... and TiledArgs::carried_in the cross section of every live record's
                                 energy in the tables of the cached view */
  bool soa_valid = true;      /* SoA arrays hold the current state */
  /* what the last step of this record store needed (0: nothing known): the next step is enqueued on
   * that assumption without a wait in between; and what share of its particles it handed to the
   * collision stage (< 0: not known; the write-back in two parts pays below a half) */
  int plan_passes = 0;
  double suspended_share = -1.0;
  unsigned final_from = 0xFFFFFFFFu; /* first slot of the graveyard (TiledArgs::sort_end) when the arrays were last
                                        current: the records from there on are dead for good, the arrays final */
  int free_count = 0; /* decomposed: slots emigrants left in the records this step */
};

struct State {
  hipStream_t stream = nullptr;
  uint64_t pid_base = 0;
  int variant = NEUTRAL_HIP_VARIANT_TILED; /* fastest on every BASELINE deck (profiles/) */
  bool variant_from_env_done = false;
  int quiet = 0;
  char tests_file[NEUTRAL_MAX_STR_LEN] = "problems/neutral.tests"; /* neutral_data.h:33 */
  NeutralHipStepStats last = {};
  /* per-device scratch, created on first use */
  int scratch_device = -1;
  neutral::StepCounters* d_counters = nullptr;
  unsigned long long* d_check = nullptr;            /* tables_check_kernel's words
                                                       (neutral_kernels.h: launch_tables_check) */
  int arithmetic = NEUTRAL_HIP_ARITH_AUTO;          /* neutral_hip_set_arithmetic */
  bool arithmetic_from_env_done = false;
  bool use_checked = false; /* auto mode: what the last step's device-side check found ... */
  const void* checked_density = nullptr; /* ... for this density mesh (another mesh starts fast) */
  bool said_checked = false;
  unsigned short* d_index[2] = {nullptr, nullptr}; /* bucketed cs indexes (scatter, absorb) */
  unsigned short* d_index_fine = nullptr;           /* finer index of the collision stage */
  hipEvent_t ev_start = nullptr;
  hipEvent_t ev_stop = nullptr;
  hipEvent_t ev_sorted = nullptr;   /* tiled variant: after the sort */
  hipEvent_t ev_streamed = nullptr; /* tiled variant: after the streaming kernel */
  hipEvent_t ev_collected = nullptr; /* tiled variant: after the collision queue is built */
  hipEvent_t ev_exported = nullptr; /* tiled variant: after the write-back to the SoA arrays */
  /* What the host reads at the step's single wait -- the two counter records, the check
   * words, the pipeline's control words, the step words -- lands in ONE block of pinned,
   * device-mapped host memory, written by one small kernel at the end of the batch: four
   * device-to-host copies into pageable memory cost 70-85 us each in the kernel trace
   * (r03/kernel_stats.csv: __amd_rocclr_copyBuffer), a quarter of a millisecond per step. */
  struct StepResults* h_results = nullptr; /* pinned host */
  struct StepResults* d_results = nullptr; /* the same block as the device sees it */
  hipStream_t comm_stream = nullptr; /* several ranks: the exchange runs here, beside the write-back */
  hipEvent_t ev_exchanged = nullptr;
  hipEvent_t ev_exchange_begins = nullptr; /* (both on comm_stream: NeutralHipStepStats.exchange_ms) */
  TableView tables;
  /* workspace of the tiled variant, grown on demand */
  neutral::TiledArgs tiled = {};
  RecordMirror mirror; /* which particle store the records mirror, and which copy is current */
  int lazy_export = 0;
  int host_syncs = 0;              /* waits for the device inside the current call */
  int exchange_rounds = 0;         /* decomposed mesh: rounds of the particle exchange in the current call */
  unsigned long long emigrants = 0; /* ... histories this rank sent away in it */
  int host_collectives = 0;        /* collectives over the ranks' host links inside the current
                                      call, the staging of the exchange itself not counted */
  unsigned long long* d_words = nullptr; /* several ranks: the step's words (event counters,
                                            flags) that travel with the tally exchange */
  /* the tallies the kernels score per cell, and the step buffers they reach the caller through
   * (MeshTally above; the energy deposition's caller is solve_transport_2d's argument) */
  MeshTally tallies[kMeshTallies] = {{1, 0, false}, {1, 0, false}, {2, 0, true}, {2, 1, true}, {4, 1, true}};
  Grown<double> susp_current; /* tiled: pending x, y sums of time-sliced histories (CurrentParams::susp), two per particle */
  Grown<double> susp_track;   /* ... and their weight * path length (scalar flux's code): TiledArgs::susp_track */
  double roulette_cutoff = 0.0;   /* neutral_hip_set_roulette: w_c, w_s (0, 0: off) */
  double roulette_survival = 0.0;
  /* neutral_hip_set_window_roulette: the kernels' view as it was set (lower null: off); filled into
   * every step's StepOptions.  Never set together with roulette_cutoff > 0. */
  neutral::WindowRouletteParams window_roulette = {};
  /* does some roulette play in the steps: their weights are summed over the ranks then */
  bool roulette_plays() const { return roulette_cutoff > 0.0 || window_roulette.lower != nullptr; }
  unsigned vacuum_sides = 0; /* neutral_hip_set_vacuum_sides: the outer sides histories escape through (0: none) */
  NeutralHipEscapeStats last_escape = {}; /* ... and what escaped in the last step, over the ranks */
  /* neutral_hip_set_periodic_axes: bit 0 x, bit 1 y (0: none); what wrapped in the last step, over
   * the ranks; and the global mesh's width and height as the steps' wraps add them (read from the
   * edge arrays by the steps that have an axis set) */
  unsigned periodic_axes = 0;
  NeutralHipWrapStats last_wraps = {};
  double periodic_width = 0.0;
  double periodic_height = 0.0;
  /* neutral_hip_set_leakage_tally: the caller's 2 * 4 * (ngroups + 1) * ncosines (null: not kept),
   * the edges as they were given, and what the steps score through: the step's buffer of as many
   * doubles and the device's copy of the edges, both made when a step first needs them (the
   * setter touches no device) */
  double* leakage_out = nullptr;
  int leakage_ngroups = 0;
  int leakage_ncosines = 1;
  double leakage_edges[neutral::kSpectrumMaxGroups + 1] = {};
  bool leakage_edges_uploaded = false;
  Grown<double> leakage_step;
  Grown<double> leakage_edges_d;
  double* leakage_scored = nullptr; /* this step: leakage_step.d when its kernels score there, else null */
  size_t leakage_bins() const { return 4 * (size_t)(leakage_ngroups + 1) * (size_t)leakage_ncosines; }
  /* neutral_hip_set_escape_bank: the caller's records (null: off) and their number; the cursor on
   * the device, made and zeroed when a step first needs it (the setter and the reset touch no
   * device: they ask the next step that records to zero it); what the host knows of it -- the
   * cursor as the last step that recorded published it, and that step's increments */
  NeutralHipEscapeRecord* bank_records = nullptr;
  uint64_t bank_capacity = 0;
  Grown<unsigned long long> bank_cursor;
  bool bank_zero_pending = false;
  bool bank_recording = false; /* this step: its kernels append to the bank */
  uint64_t bank_claimed = 0;
  uint64_t bank_step_claimed = 0, bank_step_recorded = 0;
  uint64_t bank_recorded() const { return bank_claimed < bank_capacity ? bank_claimed : bank_capacity; }
  double* d_step_scalars = nullptr; /* the step's f64 scalars (StepScalar above: kStepScalars) */
  double* spectrum_out = nullptr; /* neutral_hip_set_spectrum_tally: the caller's 2 * ngroups */
  int spectrum_ngroups = 0;       /* (null: not kept) */
  int spectrum_box[4] = {0, 0, 0, 0}; /* x0, y0, x1, y1: global cells, half-open */
  double spectrum_edges[neutral::kSpectrumMaxGroups + 1] = {};
  int auto_shard = 1;
  struct Store {
    const void* key; /* particles->x */
    int count;
    uint64_t first;
    /* decomposed mesh: the store holds whatever particles are inside this rank's
     * block right now -- `count` of `capacity` slots, keys[slot] = the particle's id */
    bool decomposed;
    int capacity;
    unsigned* keys;
  };
  /* spatial domain decomposition (neutral_hip_set_decomposition) */
  bool domain_on = false;
  neutral::DomainGrid domain = {1, 1, 0, 0};
  double source_box[4] = {0.0, 0.0, 0.0, 0.0};
  bool source_box_set = false;
  unsigned* d_exchange = nullptr;    /* counts[64], offsets[64], cursors[64], 1 compaction cursor */
  Grown<neutral::ParticleRec> send; /* the particle exchange's records, out and in */
  Grown<neutral::ParticleRec> recv;
  Grown<unsigned> free_slots; /* slots emigrants left in this step (arrivals reuse them: RecordMirror::holes) */
  enum { kMaxStores = 64 };
  Store stores[kMaxStores] = {};
  int nstores = 0;
  /* mesh extent: only for the tiled variant's "facets still ahead" estimate */
  double mesh_width = 1.0;
  double mesh_height = 1.0;
  const void* extent_edges = nullptr;
  double edge_dx = 0.0; /* the caller's edgedx[pad] / edgedy[pad] for the same mesh (0: none) */
  double edge_dy = 0.0;
  int extent_nx = 0;
  int extent_ny = 0;
  int tiled_particles = 0;
  int tiled_tiles = 0;
  Grown<uint4> chunks; /* TiledArgs::chunks */
  /* the write-back split in two (neutral_kernels.h: SplitExport): the stream its first part runs
   * on beside the collision stage, its event (the share of the particles that decides on it:
   * RecordMirror::last_suspended_share) */
  hipStream_t export_stream = nullptr;
  hipEvent_t ev_split_done = nullptr;
  neutral::ParticleView* d_export_view = nullptr; /* the stepped store's array pointers, for the */
  neutral::ParticleView h_export_view = {};        /* collision stage's own write-back */
  bool export_view_uploaded = false;
  size_t susp_id_words = 0;
  neutral::LaunchTuning tuning = {}; /* read once per store (neutral_kernels.h) */
  bool tuning_read = false;
  Grown<char> census; /* the operations between two steps share one workspace (neutral_comb.hip: Rooms):
                         bytes, grown to what a call asks for, freed with a store */
  int stream_queues = 0;   /* neutral_hip_set_stream_queues: the stream kernel's tile queues are in use */
  size_t queue_places = 0; /* ... places allocated, for how many tiles */
  int queue_tiles = 0;
};

extern State g;

/* What the ranks need of each other per batch of launches besides the tally: the event
 * counters and the flags every rank must act on together (an attempt turned down, stream
 * passes still owed).  Packed on the device, summed by the same transport as the tally on
 * the same stream, read with the batch's single wait: a steady-state step makes no
 * collective over the host links of its own. */
enum StepWord : int {
  kWordCounters = 0,   /* 2 x {nprocessed, nfacets, ncollisions, ncensus} */
  kWordRequeued = 8,
  kWordCollidePasses = 9,
  kWordTurnedDown = 10, /* ranks whose attempt was turned down on the device */
  kWordMigrants = 11,   /* histories still waiting for a stream pass */
  kWordQueued = 12,     /* histories this batch's collision stage was handed */
  kWordAborted = 13,
  kWordRanks = 14,      /* 1 per rank: how many ranks the transport summed over */
  kWordSteals = 15,     /* rings the collision stage's waves took from (see StepCounters) */
  kWordStealsRefused = 16, /* waves that found their CU list overfull and stole nothing */
  kWordWeightedWaves = 17, /* waves of the collision stage that were dealt a weighted share */
  kWordRouletteKilled = 18,   /* Russian roulette: histories it ended ... */
  kWordRouletteSurvived = 19, /* ... and kept (the weights: StepScalar) */
  kStepWords = 20,
};

/* ---- neutral_abi_store.hip ---- */
void ensure_scratch();
void read_variant_env();
void wait_for_stream(); /* every wait for the device goes through here: NeutralHipStepStats.host_syncs */
void* device_zalloc(size_t bytes);
void ensure_tiled_workspace(int nx, int ny, int nparticles_now, int capacity);
void before_device_write(const void* dst, size_t bytes);
void refresh_table_view(const NeutralHipCrossSection* cs_s, const NeutralHipCrossSection* cs_a,
                        bool force, bool fast_arithmetic);
neutral::ParticleView view_of(const NeutralHipParticle* p);
const State::Store* find_store(const NeutralHipParticle* p);
State::Store* remember_store(const NeutralHipParticle* p, int count, uint64_t first);
void forget_store(const NeutralHipParticle* p);
/* is the scalar flux's code in use: for the caller's flux mesh, or for the current's or the
 * outflow's sake (which a vacuum side or a periodic axis turns on: begin_step_scoring)? */
inline bool flux_code_on() {
  return g.tallies[kTallyFlux].caller[0] != nullptr || g.tallies[kTallyCurrent].caller[0] != nullptr ||
         g.tallies[kTallyOutflow].caller[0] != nullptr || g.vacuum_sides != 0 || g.periodic_axes != 0;
}
/* The step's optional scoring as its launches take it (neutral_kernels.h), from what the
 * neutral_hip_set_* calls left; the step buffers of the tallies that go through one, cleared
 * on the caller's stream; a.tally and a.flux_tally where this step's kernels score. */
neutral::StepOptions begin_step_scoring(neutral::SolveArgs& a, double* energy_tally, bool tiled,
                                        bool exchange);
void run_inject(const int nparticles, const int local_nx, const int local_ny, const int pad,
                const double left_off, const double bottom_off, const double width,
                const double height, const int x_off, const int y_off, const double dt,
                const double* edgex, const double* edgey, const double initial_energy,
                const NeutralHipParticle* particles);
void run_inject_filtered(State::Store* st, const int nparticles, const int local_nx,
                         const int local_ny, const int pad, const double left_off,
                         const double bottom_off, const double width, const double height,
                         const int x_off, const int y_off, const double dt, const double* edgex,
                         const double* edgey, const double initial_energy,
                         const NeutralHipParticle* particles);

/* ---- neutral_abi_exchange.hip ---- */
void exchange_step(const neutral::SolveArgs& a, bool tiled);
/* one rank, or a decomposed mesh (every rank its own cells: nothing to sum over the ranks): the
 * step buffers into the caller's arrays, on the caller's stream */
void tallies_to_caller(const neutral::SolveArgs& a);
void finish_exchange();
void publish_results(bool tiled, bool with_words);
void fetch_results(neutral::StepCounters* hc, unsigned long long* check, unsigned* ctrl,
                   unsigned long long* words);
int exchange_particles(const neutral::SolveArgs& a, neutral::TiledArgs& t);

}  // namespace neutral_abi
#endif
