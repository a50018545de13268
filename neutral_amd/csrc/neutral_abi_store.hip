/*
 * neutral_abi_store.hip -- particle stores, the tiled variant's workspace and the records that
 * mirror a store's SoA arrays, the cached view of the cross-section tables, the HBM flavour of
 * the reference's allocation / copy hooks, settings and probes (include/neutral_hip.h, sections
 * 2 and 3).  Host code only.
 */
#include "neutral_abi_state.h"

namespace neutral_abi {

State g;


void ensure_scratch() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  if (g.scratch_device == dev) {
    return;
  }
  /* scratch of another device (if any) is abandoned: a process drives one GPU */
  HIP_CHECK(hipMalloc((void**)&g.d_counters, 2 * sizeof(neutral::StepCounters)));
  HIP_CHECK(hipMalloc((void**)&g.d_check, 16 * sizeof(unsigned long long)));
  HIP_CHECK(hipMemset(g.d_check, 0, 16 * sizeof(unsigned long long))); /* ([8..12]: accumulators) */
  HIP_CHECK(hipMalloc((void**)&g.d_exchange, sizeof(unsigned) * 200));
  HIP_CHECK(hipMalloc((void**)&g.d_words, sizeof(unsigned long long) * kStepWords));
  HIP_CHECK(hipMalloc((void**)&g.d_step_scalars, kStepScalars * sizeof(double)));
  g.tables.valid = false; /* its indexes live in the other device's scratch */
  HIP_CHECK(hipMalloc((void**)&g.d_index_fine,
                      sizeof(unsigned short) * (kMaxFineIndexBuckets + 1)));
  for (unsigned short*& d : g.d_index) {
    HIP_CHECK(hipMalloc((void**)&d, sizeof(unsigned short) * (kMaxIndexBuckets + 1)));
  }
  HIP_CHECK(hipEventCreate(&g.ev_start));
  HIP_CHECK(hipEventCreate(&g.ev_stop));
  HIP_CHECK(hipEventCreate(&g.ev_sorted));
  HIP_CHECK(hipEventCreate(&g.ev_streamed));
  HIP_CHECK(hipEventCreate(&g.ev_collected));
  HIP_CHECK(hipEventCreate(&g.ev_exported));
  HIP_CHECK(hipEventCreate(&g.ev_exchanged));
  HIP_CHECK(hipEventCreate(&g.ev_exchange_begins));
  HIP_CHECK(hipStreamCreateWithFlags(&g.comm_stream, hipStreamNonBlocking));
  {
    /* (lowest priority: what runs there gets the CUs the caller's stream leaves free) */
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_CHECK(hipStreamCreateWithPriority(&g.export_stream, hipStreamNonBlocking, least));
    HIP_CHECK(hipEventCreateWithFlags(&g.ev_split_done, hipEventDisableTiming));
    HIP_CHECK(hipMalloc((void**)&g.d_export_view, sizeof(neutral::ParticleView)));
    g.export_view_uploaded = false;
  }
  if (!g.h_results) {
    HIP_CHECK(hipHostMalloc((void**)&g.h_results, sizeof(StepResults), hipHostMallocMapped));
    memset(g.h_results, 0, sizeof(StepResults));
  }
  HIP_CHECK(hipHostGetDevicePointer((void**)&g.d_results, g.h_results, 0));
  g.scratch_device = dev;
}

/* NEUTRAL_HIP_VARIANT and NEUTRAL_HIP_ARITH, each read once unless an explicit choice came first */
void read_variant_env() {
  if (!g.variant_from_env_done) {
    g.variant_from_env_done = true;
    const char* v = getenv("NEUTRAL_HIP_VARIANT");
    if (v && *v) {
      const int iv = atoi(v);
      if (iv == NEUTRAL_HIP_VARIANT_OVER_PARTICLE || iv == NEUTRAL_HIP_VARIANT_EVENT_SORTED ||
          iv == NEUTRAL_HIP_VARIANT_TILED) {
        g.variant = iv;
      } else {
        fprintf(stderr, "libneutral_hip: ignoring NEUTRAL_HIP_VARIANT=%s\n", v);
      }
    }
  }
  if (!g.arithmetic_from_env_done) {
    g.arithmetic_from_env_done = true;
    const char* arith = getenv("NEUTRAL_HIP_ARITH");
    if (arith && strcmp(arith, "checked") == 0) {
      g.arithmetic = NEUTRAL_HIP_ARITH_CHECKED;
    }
  }
}

/* every wait for the device goes through here: NeutralHipStepStats.host_syncs */
void wait_for_stream() {
  HIP_CHECK(hipStreamSynchronize(g.stream));
  g.host_syncs++;
}

void* device_zalloc(size_t bytes) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1));
  HIP_CHECK(hipMemsetAsync(p, 0, bytes ? bytes : 1, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  return p;
}

/* Builds the exponent-bucketed index of one key array into d_start (see
 * neutral_device.h).  Returns a null index when the table cannot be indexed:
 * more than 65 535 entries (u16 starts) or non-positive first key (bit patterns
 * of non-positive doubles do not order like their values). */
neutral::CsIndex build_index(const double* d_keys, int n, unsigned short* d_start,
                             int first_shift = 44 /* 256 buckets per binade */,
                             int max_buckets = kMaxIndexBuckets) {
  neutral::CsIndex ix = {nullptr, 0, 0, 0};
  if (n < 2 || n > 65535) {
    return ix;
  }
  double ends[2];
  HIP_CHECK(hipMemcpyAsync(&ends[0], d_keys, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&ends[1], d_keys + (n - 1), sizeof(double), hipMemcpyDeviceToHost,
                           g.stream));
  wait_for_stream();
  if (!(ends[0] > 0.0) || !(ends[1] > ends[0])) {
    return ix;
  }
  long long lo_bits, hi_bits;
  memcpy(&lo_bits, &ends[0], sizeof(lo_bits));
  memcpy(&hi_bits, &ends[1], sizeof(hi_bits));
  int shift = first_shift;
  while (((hi_bits >> shift) - (lo_bits >> shift) + 1) > max_buckets) {
    shift++;
  }
  ix.shift = shift;
  ix.base = lo_bits >> shift;
  ix.nbuckets = (int)((hi_bits >> shift) - ix.base + 1);
  HIP_CHECK(neutral::launch_build_cs_index(d_keys, n, ix.shift, ix.base, ix.nbuckets, d_start,
                                           g.stream));
  ix.start = d_start;
  return ix;
}

/* Writes the records back to the SoA store they mirror if they are ahead of it. */
void RecordMirror::write_back() {
  if (!soa_valid && rec_valid && rec_owner) {
    if (rec_owner_keys) { /* decomposed mesh: slot for slot */
      HIP_CHECK(neutral::launch_export_by_slot(g.tiled.rec_in, rec_owner_view, rec_owner_keys, rec_count,
                                               g.stream));
    } else {
      /* (slot_of_id is kept by every step, lazy or not: the kernels that place a record note
       * where -- 0.3 ms per step at 1e8 -- and the write-back on demand costs what the pass
       * inside a step costs, not twice that for reading the ids out of the records first) */
      HIP_CHECK(neutral::launch_export_records(g.tiled.rec_in, g.tiled.slot_of_id, rec_owner_view,
                                               rec_count, g.stream, nullptr, nullptr, final_from));
      final_from = (unsigned)g.tiled.sort_end; /* (the graveyard as of now: final in the arrays) */
    }
    wait_for_stream();
  }
  soa_valid = true;
}

bool RecordMirror::overlaps(const void* p, size_t bytes) const {
  if (!rec_owner || !rec_valid) {
    return false;
  }
  const neutral::ParticleView& v = rec_owner_view;
  const size_t n = (size_t)rec_count;
  const char* lo = (const char*)p;
  const char* hi = lo + bytes;
  const void* f64[] = {v.x, v.y, v.omega_x, v.omega_y, v.energy, v.weight, v.dt_to_census,
                       v.mfp_to_collision};
  for (const void* a : f64) {
    if (lo < (const char*)a + sizeof(double) * n && hi > (const char*)a) return true;
  }
  const void* i32[] = {v.cellx, v.celly, v.dead};
  for (const void* a : i32) {
    if (lo < (const char*)a + sizeof(int) * n && hi > (const char*)a) return true;
  }
  return false;
}

/* (Re)allocates the tiled variant's workspace for this problem size. */
void ensure_tiled_workspace(int nx, int ny, int nparticles_now, int capacity) {
  /* (a decomposed store can grow up to its capacity within a step: buffers are sized
   * for that, the tile edge for what is there now) */
  int tx, ty, max_chunks;
  const int shift = neutral::tiled_tile_shift(nx, ny, nparticles_now, flux_code_on());
  const int nparticles = capacity > nparticles_now ? capacity : nparticles_now;
  neutral::tiled_geometry(nx, ny, nparticles, shift, &tx, &ty, &max_chunks);
  neutral::TiledArgs& t = g.tiled;
  const bool grow = nparticles > g.tiled_particles || tx * ty > g.tiled_tiles;
  if (grow || shift != t.tile_shift || tx != t.tiles_x || ty != t.tiles_y) {
    /* the record summaries hold tile numbers of the old geometry, and the buffers
     * may be about to go: a pending write-back of their owner comes first */
    g.mirror.write_back();
    g.mirror.drop();
  }
  /* what time-sliced histories have pending, for the workspace's particles (the old ones unless it
   * grows): either buffer may have missed a growth that happened while its tally was off */
  const size_t cap = (size_t)(grow ? nparticles : g.tiled_particles);
  if (g.tallies[kTallyCurrent].caller[0]) { /* the current, x and y */
    ensure_capacity(g.susp_current, (size_t)g.tiled_particles, cap, 2 * sizeof(double), grow || !g.susp_current.d);
  }
  if (flux_code_on()) { /* weight * path length */
    ensure_capacity(g.susp_track, (size_t)g.tiled_particles, cap, sizeof(double), grow || !g.susp_track.d);
    t.susp_track = g.susp_track.d;
  }
  if (grow) {
    void* old[] = {t.order,  t.collide_queue, t.tile_count, t.tile_offset, t.tile_cursor, t.rec_in,
                   t.rec_out, t.info_in,      t.info_out,   t.susp,        t.id_in,       t.id_out,
                   t.slot_of_id, t.tile_uniform, t.carried_in, t.carried_out};
    for (void* p : old) {
      if (p) HIP_CHECK(hipFree(p));
    }
    const size_t n = (size_t)nparticles;
    const size_t nb = (size_t)(tx * ty * 4 + 2); /* (up to four reach classes per tile) */
    HIP_CHECK(hipMalloc((void**)&t.order, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.collide_queue, sizeof(unsigned) * n));
    if (t.susp_ids) HIP_CHECK(hipFree(t.susp_ids));
    g.susp_id_words = (n + 31) / 32;
    HIP_CHECK(hipMalloc((void**)&t.susp_ids, sizeof(unsigned) * g.susp_id_words));
    HIP_CHECK(hipMalloc((void**)&t.rec_in, sizeof(neutral::ParticleRec) * n));
    HIP_CHECK(hipMalloc((void**)&t.rec_out, sizeof(neutral::ParticleRec) * n));
    HIP_CHECK(hipMalloc((void**)&t.info_in, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.info_out, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.id_in, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.id_out, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.slot_of_id, sizeof(unsigned) * n));
    HIP_CHECK(hipMalloc((void**)&t.carried_in, sizeof(neutral::CarriedStart) * n));
    HIP_CHECK(hipMalloc((void**)&t.carried_out, sizeof(neutral::CarriedStart) * n));
    HIP_CHECK(hipMalloc((void**)&t.susp, sizeof(neutral::SuspendExtra) * n));
    HIP_CHECK(hipMalloc((void**)&t.tile_count, sizeof(unsigned) * nb));
    HIP_CHECK(hipMalloc((void**)&t.tile_offset, sizeof(unsigned) * nb));
    HIP_CHECK(hipMalloc((void**)&t.tile_cursor, sizeof(unsigned) * nb));
    HIP_CHECK(hipMalloc((void**)&t.tile_uniform, (size_t)(tx * ty + 1)));
    HIP_CHECK(hipMemsetAsync(t.tile_uniform, 0, (size_t)(tx * ty + 1), g.stream));
    g.tiled_particles = nparticles;
    g.tiled_tiles = tx * ty;
  }
  /* the counting sort expects its histogram zeroed (it clears what it consumes) */
  HIP_CHECK(hipMemsetAsync(t.tile_count, 0, sizeof(unsigned) * (size_t)(tx * ty * 4 + 2), g.stream));
  ensure_capacity(g.chunks, (size_t)max_chunks, (size_t)max_chunks);
  t.chunks = g.chunks.d;
  if (!t.steal) {
    /* rings' control words and CU lists of the collision stage's stealing: they belong to
     * this workspace and are reset by a kernel of the launch that uses them */
    t.steal = (neutral::StealWork*)device_zalloc(sizeof(neutral::StealWork));
  }
  if (!t.ctrl) {
    HIP_CHECK(hipMalloc((void**)&t.ctrl, sizeof(unsigned) * 16));
    HIP_CHECK(hipMemsetAsync(t.ctrl, 0, sizeof(unsigned) * 16, g.stream));
    HIP_CHECK(hipMalloc((void**)&t.edges_computed, sizeof(int)));
    HIP_CHECK(hipMemsetAsync(t.edges_computed, 0, sizeof(int), g.stream));
  }
  t.tile_shift = shift;
  t.window_min_particles = neutral::tiled_window_min_particles(shift);
  t.tiles_x = tx;
  t.tiles_y = ty;
  t.ntiles = tx * ty;
  /* Sparse problems (about a workgroup's worth of particles per tile and pass, or fewer)
   * also sort by reach class inside a tile (neutral_history.h: reach_class); where tiles hold
   * tens of thousands, lanes are refilled from the chunk and the order inside it does not
   * matter.  NEUTRAL_REACH_CLASSES=1|4 overrides. */
  {
    const long long per_tile = (long long)nparticles_now / (tx * ty > 0 ? tx * ty : 1);
    /* (and only while the buckets still fit the sort's LDS histogram: 8 192) */
    int classes = (per_tile < 8192 && (long long)tx * ty * 4 + 1 <= 8192) ? 4 : 1;
    const char* force = getenv("NEUTRAL_REACH_CLASSES");
    if (force && (atoi(force) == 1 || atoi(force) == 4)) {
      classes = atoi(force);
    }
    if (classes != t.reach_classes && t.reach_classes != 0) {
      g.mirror.write_back();
      g.mirror.drop(); /* (the summaries' class field changes meaning) */
    }
    t.reach_classes = classes;
    t.nsort = t.ntiles * classes;
  }
  t.max_chunks = max_chunks;
  /* The stream kernel's tile queues: a log per tile, sized for what a tile can receive in one
   * launch -- every particle once (a source box inside one tile sends them all through its
   * neighbours), at least 4 096 places, 4 GiB of logs at most, of which only what is used is ever
   * touched (a tile that receives more overflows into the pass mechanism:
   * NeutralHipStepStats.stream_overflows).
   * Off by default (measured: at best level with the pass mechanism, slower on sparse decks --
   * DESIGN.md section 4 item 12); neutral_hip_set_stream_queues(1) or NEUTRAL_STREAM_QUEUES=1
   * turn them on. */
  {
    const char* switch_env = getenv("NEUTRAL_STREAM_QUEUES");
    const bool off = !(switch_env ? atoi(switch_env) != 0 : g.stream_queues != 0);
    size_t cap = ((size_t)nparticles + 1023) & ~(size_t)1023;
    cap = cap < 4096 ? 4096 : (cap > ((size_t)1 << 22) ? ((size_t)1 << 22) : cap);
    while ((size_t)t.ntiles * cap * sizeof(unsigned) > ((size_t)4 << 30) && cap > 1024) {
      cap >>= 1;
    }
    if (const char* force = getenv("NEUTRAL_STREAM_QUEUE_CAPACITY")) { /* (tests: overflow) */
      if (atoi(force) > 0) cap = (size_t)atoi(force);
    }
    const size_t want = off ? 0 : (size_t)t.ntiles * cap;
    if (want != g.queue_places || (int)t.ntiles != g.queue_tiles) {
      if (t.queue_entries) HIP_CHECK(hipFree(t.queue_entries));
      if (t.queue_tail) HIP_CHECK(hipFree(t.queue_tail));
      if (t.queue_head) HIP_CHECK(hipFree(t.queue_head));
      t.queue_entries = t.queue_tail = t.queue_head = nullptr;
      if (want) {
        HIP_CHECK(hipMalloc((void**)&t.queue_entries, sizeof(unsigned) * want));
        HIP_CHECK(hipMemsetAsync(t.queue_entries, 0xFF, sizeof(unsigned) * want, g.stream));
        t.queue_tail = (unsigned*)device_zalloc(sizeof(unsigned) * (size_t)t.ntiles);
        t.queue_head = (unsigned*)device_zalloc(sizeof(unsigned) * (size_t)t.ntiles);
      }
      g.queue_places = want;
      g.queue_tiles = t.ntiles;
    }
    t.queue_capacity = (unsigned)cap;
  }
}

/* a caller is about to overwrite device memory through one of the library's own
 * copy hooks: if it is part of the mirrored particle store, the store becomes the
 * truth again (pending record state is written back first, so a partial overwrite
 * keeps the rest) */
void before_device_write(const void* dst, size_t bytes) {
  if (g.mirror.overlaps(dst, bytes)) {
    g.mirror.write_back();
    g.mirror.drop();
  }
}

/* What the library derives from the cs tables (see TableView).  Builds the view when
 * the tables (pointers, sizes, variant) are new -- that waits for the device -- and
 * otherwise only enqueues the device-side check of the contents. */
void refresh_table_view(const NeutralHipCrossSection* cs_s, const NeutralHipCrossSection* cs_a,
                        bool rebuild, bool fast_arithmetic) {
  TableView& v = g.tables;
  const bool same_args = v.valid && v.keys_s == cs_s->keys && v.values_s == cs_s->values &&
                         v.n_s == cs_s->nentries && v.keys_a == cs_a->keys &&
                         v.values_a == cs_a->values && v.n_a == cs_a->nentries &&
                         v.variant == g.variant;
  if (!same_args || rebuild) {
    v.valid = false;
    g.mirror.tables_changed(); /* (the records' carried cross sections were looked up in other tables) */
    v.keys_s = cs_s->keys;
    v.values_s = cs_s->values;
    v.n_s = cs_s->nentries;
    v.keys_a = cs_a->keys;
    v.values_a = cs_a->values;
    v.n_a = cs_a->nentries;
    v.variant = g.variant;
    /* identity and key hashes from the check kernel itself (expectations unknown) */
    HIP_CHECK(neutral::launch_tables_check(v.keys_s, v.values_s, v.n_s, v.keys_a, v.values_a, v.n_a,
                                           0ull, 0ull, -1, 0, g.d_check, g.stream));
    unsigned long long h[4];
    HIP_CHECK(hipMemcpyAsync(h, g.d_check, sizeof(h), hipMemcpyDeviceToHost, g.stream));
    wait_for_stream();
    v.hash_s = h[1];
    v.hash_a = h[2];
    v.same = (int)h[3];
    /* bucketed indexes */
    v.ix_s = build_index(v.keys_s, v.n_s, g.d_index[0]);
    v.ix_a = v.ix_s;
    if (!v.same) {
      v.ix_a = build_index(v.keys_a, v.n_a, g.d_index[1]);
      if (v.ix_a.start && v.ix_s.start && v.ix_a.shift != v.ix_s.shift) {
        v.ix_a.start = nullptr; /* one shift per launch: the absorb table falls back to bisection */
      }
      if (!v.ix_s.start && v.ix_a.start) {
        v.ix_s.shift = v.ix_a.shift;
      }
    }
    v.fine = {nullptr, 0, 0, 0};
    /* (NEUTRAL_NO_FINE_INDEX=1: experiments that need the collision stage's workgroups small in
     * LDS -- 17 KB instead of 34 -- to sit beside another kernel's; read once per view) */
    const char* no_fine = getenv("NEUTRAL_NO_FINE_INDEX");
    if (v.same && v.ix_s.start && g.variant == NEUTRAL_HIP_VARIANT_TILED && !(no_fine && atoi(no_fine) != 0)) {
      const neutral::CsIndex fine =
          build_index(v.keys_s, v.n_s, g.d_index_fine, 43, kMaxFineIndexBuckets);
      if (fine.start && fine.shift < v.ix_s.shift) {
        v.fine = fine;
      }
    }
    v.valid = true;
  }
  /* every step: the contents against the view (result read with the step's counters) */
  HIP_CHECK(neutral::launch_tables_check(v.keys_s, v.values_s, v.n_s, v.keys_a, v.values_a, v.n_a,
                                         v.hash_s, v.hash_a, v.same, fast_arithmetic ? 1 : 0,
                                         g.d_check, g.stream));
}

neutral::ParticleView view_of(const NeutralHipParticle* p) {
  neutral::ParticleView v;
  v.x = p->x;
  v.y = p->y;
  v.omega_x = p->omega_x;
  v.omega_y = p->omega_y;
  v.energy = p->energy;
  v.weight = p->weight;
  v.dt_to_census = p->dt_to_census;
  v.mfp_to_collision = p->mfp_to_collision;
  v.cellx = p->cellx;
  v.celly = p->celly;
  v.dead = p->dead;
  return v;
}

const State::Store* find_store(const NeutralHipParticle* p) {
  for (int i = 0; i < g.nstores; ++i) {
    if (p && g.stores[i].key == (const void*)p->x) {
      return &g.stores[i];
    }
  }
  return nullptr;
}

State::Store* remember_store(const NeutralHipParticle* p, int count, uint64_t first) {
  if (g.nstores == State::kMaxStores) {
    fprintf(stderr, "libneutral_hip: more than %d sharded particle stores alive at once "
                    "(neutral_hip_free_particles releases one).\n", (int)State::kMaxStores);
    exit(EXIT_FAILURE);
  }
  const int slot = g.nstores++;
  g.stores[slot] = State::Store{(const void*)p->x, count, first, false, count, nullptr};
  return &g.stores[slot];
}

void forget_store(const NeutralHipParticle* p) {
  for (int i = 0; i < g.nstores; ++i) {
    if (g.stores[i].key == (const void*)p->x) {
      if (g.stores[i].keys) HIP_CHECK(hipFree(g.stores[i].keys));
      g.stores[i] = g.stores[--g.nstores];
      return;
    }
  }
}

/* the tally's step buffer for a mesh of ncells, grown on demand and cleared on the caller's stream */
static double* step_meshes(MeshTally& t, size_t ncells) {
  if (ensure_capacity(t.step, ncells, ncells, sizeof(double) * (size_t)(t.meshes + t.spare_meshes))) {
    HIP_CHECK(hipMemsetAsync(t.step.d + ncells * (size_t)t.meshes, 0,
                             sizeof(double) * ncells * (size_t)t.spare_meshes, g.stream));
  }
  HIP_CHECK(hipMemsetAsync(t.step.d, 0, sizeof(double) * ncells * (size_t)t.meshes, g.stream));
  return t.step.d;
}

neutral::StepOptions begin_step_scoring(neutral::SolveArgs& a, double* energy_tally, bool tiled,
                                        bool exchange) {
  const size_t ncells = (size_t)a.nx * (size_t)a.ny;
  g.tallies[kTallyEnergy].caller[0] = energy_tally;
  if (MeshTally& out = g.tallies[kTallyOutflow]; out.caller[0]) {
    for (int m = 1; m < out.meshes; ++m) {
      out.caller[m] = out.caller[0] + (size_t)m * ncells; /* (one caller buffer: neutral_hip.h) */
    }
  }
  for (MeshTally& t : g.tallies) {
    t.scored = (t.caller[0] && (t.always_buffered || exchange)) ? step_meshes(t, ncells) : nullptr;
  }
  if (MeshTally& out = g.tallies[kTallyOutflow]; (g.vacuum_sides != 0 || g.periodic_axes != 0) && !out.scored) {
    /* vacuum sides and periodic axes ride the instantiations that score the outflow: without a
     * caller's mesh the step's buffer is scored and added to nothing (step_buffers_to_caller) */
    out.scored = step_meshes(out, ncells);
  }
  a.tally = exchange ? g.tallies[kTallyEnergy].scored : energy_tally;
  a.flux_tally = exchange ? g.tallies[kTallyFlux].scored : g.tallies[kTallyFlux].caller[0];
  neutral::StepOptions o;
  o.collision_tallies = g.tallies[kTallyCollisions].scored;
  o.roulette_cutoff = g.roulette_cutoff;
  o.roulette_survival = g.roulette_survival;
  if (g.window_roulette.lower) {
    /* (the bins are global cells of the mesh the window was set for: a step on another mesh does
     * not run -- neutral_hip.h) */
    if (a.global_nx != g.window_roulette.nx || a.global_ny != g.window_roulette.ny) {
      fprintf(stderr,
              "libneutral_hip: solve_transport_2d on a global mesh of %d x %d, but "
              "neutral_hip_set_window_roulette was given %d x %d.\n",
              a.global_nx, a.global_ny, g.window_roulette.nx, g.window_roulette.ny);
      exit(EXIT_FAILURE);
    }
    o.window = g.window_roulette;
  }
  if (g.spectrum_out) {
    /* (its step buffer follows the two roulette weights, so that with several ranks sharing the
     * mesh the spectrum rides their all-reduce: exchange_step) */
    neutral::SpectrumParams& sp = o.spectrum;
    sp.buffer = g.d_step_scalars + kScalarSpectrum;
    HIP_CHECK(hipMemsetAsync(sp.buffer, 0, 2 * sizeof(double) * (size_t)g.spectrum_ngroups, g.stream));
    sp.ngroups = g.spectrum_ngroups;
    sp.x0 = g.spectrum_box[0];
    sp.y0 = g.spectrum_box[1];
    sp.width = (unsigned)(g.spectrum_box[2] - g.spectrum_box[0]);
    sp.height = (unsigned)(g.spectrum_box[3] - g.spectrum_box[1]);
    for (int i = 0; i <= g.spectrum_ngroups; ++i) {
      sp.edges[i] = g.spectrum_edges[i];
    }
  }
  if (double* const jx = g.tallies[kTallyCurrent].scored) {
    o.current = {jx, jx + ncells, tiled ? g.susp_current.d : nullptr};
    if (!a.flux_tally) {
      a.flux_tally = jx + 2 * ncells; /* (the flux code it runs scores into the mesh nobody reads) */
    }
  }
  if (double* const out = g.tallies[kTallyOutflow].scored) {
    o.outflow = out;
    if (!a.flux_tally) {
      a.flux_tally = out + 4 * ncells; /* (likewise) */
    }
  }
  o.vacuum_sides = g.vacuum_sides;
  if (g.periodic_axes != 0) {
    if (a.decomposed) {
      /* (a block of the mesh: solve_transport_2d has had the ranks agree on the extent for this step) */
      o.periodic = {g.periodic_axes, 0u, g.periodic_width, g.periodic_height, {nullptr, nullptr, nullptr, nullptr}};
    } else {
      /* (the whole mesh is this rank's: its extent is worked out on the device, where the options
       * are stored -- the edge arrays may be anyone's and may have changed since the last step) */
      o.periodic = {g.periodic_axes, 0u, 0.0, 0.0,
                    {a.edgex + a.pad, a.edgex + a.pad + a.nx, a.edgey + a.pad, a.edgey + a.pad + a.ny}};
    }
  }
  g.leakage_scored = nullptr;
  if (g.leakage_out && g.vacuum_sides != 0) {
    /* (nothing escapes while no side is vacuum: the step then runs what it runs without the tally) */
    const size_t n = 2 * g.leakage_bins();
    ensure_capacity(g.leakage_step, n, n);
    HIP_CHECK(hipMemsetAsync(g.leakage_step.d, 0, sizeof(double) * n, g.stream));
    if (g.leakage_ngroups > 0 && !g.leakage_edges_uploaded) {
      ensure_capacity(g.leakage_edges_d, (size_t)neutral::kSpectrumMaxGroups + 1, (size_t)neutral::kSpectrumMaxGroups + 1);
      HIP_CHECK(hipMemcpyAsync(g.leakage_edges_d.d, g.leakage_edges, sizeof(double) * (size_t)(g.leakage_ngroups + 1),
                               hipMemcpyHostToDevice, g.stream));
      g.leakage_edges_uploaded = true;
    }
    g.leakage_scored = g.leakage_step.d;
    o.leakage = {g.leakage_step.d, g.leakage_ngroups > 0 ? g.leakage_edges_d.d : nullptr, g.leakage_ngroups,
                 g.leakage_ncosines};
  }
  g.bank_recording = false;
  if (g.bank_records && g.vacuum_sides != 0 && !a.decomposed) {
    /* (a decomposed store: the step runs as without the bank -- neutral_hip.h) */
    if (ensure_capacity(g.bank_cursor, 1, 1) || g.bank_zero_pending) {
      HIP_CHECK(hipMemsetAsync(g.bank_cursor.d, 0, sizeof(unsigned long long), g.stream));
      g.bank_zero_pending = false;
    }
    g.bank_recording = true;
    o.bank = {(neutral::EscapeRecord*)g.bank_records, g.bank_cursor.d, (unsigned long long)g.bank_capacity};
  }
  return o;
}

struct Shard {
  int n;             /* this rank's shard, whatever count the caller names */
  uint64_t pid_base;
};

/* the shard and the mesh it emits into; the injectors and the fixed source also name a box (left, bottom,
 * width, height) and an energy */
static neutral::InjectArgs inject_args(const Shard& s, const NeutralHipParticle* particles, int local_nx, int local_ny,
                                       int pad, int x_off, int y_off, double dt, const double* edgex,
                                       const double* edgey, const double* box = nullptr, double energy = 0.0) {
  const double none[4] = {0.0, 0.0, 0.0, 0.0};
  const double* b = box ? box : none;
  return neutral::InjectArgs{s.n, s.pid_base, local_nx, local_ny, pad, x_off, y_off, b[0],
                             b[1], b[2],      b[3],     dt,       energy, edgex, edgey, view_of(particles)};
}

void run_inject(const int nparticles, const int local_nx, const int local_ny, const int pad,
                const double left_off, const double bottom_off, const double width,
                const double height, const int x_off, const int y_off, const double dt,
                const double* edgex, const double* edgey, const double initial_energy,
                const NeutralHipParticle* particles) {
  const double box[4] = {left_off, bottom_off, width, height};
  const neutral::InjectArgs a = inject_args(Shard{nparticles, g.pid_base}, particles, local_nx, local_ny, pad, x_off,
                                            y_off, dt, edgex, edgey, box, initial_energy);
  g.mirror.arrays_rewritten(particles, /*whole_store=*/true);
  HIP_CHECK(neutral::launch_inject(a, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

/* decomposed mesh: this rank's part of the injected particles (see inject_particles) */
void run_inject_filtered(State::Store* st, const int nparticles, const int local_nx,
                         const int local_ny, const int pad, const double left_off,
                         const double bottom_off, const double width, const double height,
                         const int x_off, const int y_off, const double dt, const double* edgex,
                         const double* edgey, const double initial_energy,
                         const NeutralHipParticle* particles) {
  ensure_scratch();
  /* the global source box, if the caller named it (neutral_hip_set_source_box);
   * otherwise the box passed in is taken to be it */
  const double given[4] = {left_off, bottom_off, width, height};
  const neutral::InjectArgs a =
      inject_args(Shard{nparticles, 0}, particles, local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey,
                  g.source_box_set ? g.source_box : given, initial_energy);
  g.mirror.arrays_rewritten(particles, /*whole_store=*/true);
  unsigned kept = 0;
  HIP_CHECK(neutral::launch_inject_filtered(a, st->keys, g.d_exchange + 192, g.stream));
  HIP_CHECK(hipMemcpyAsync(&kept, g.d_exchange + 192, sizeof(unsigned), hipMemcpyDeviceToHost,
                           g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  st->count = (int)kept;
}

}  // namespace neutral_abi

using namespace neutral_abi;

/* ---- comb, source, window: what the three calls between two timesteps share ------------------ */
namespace {

/* The prologue: *stats zeroed, then -> 0 and the shard that `particles` names, or the call's return
 * code: 2 for a decomposed store, 1 where there is nothing to work on.  Nothing else is touched. */
template <class Stats>
int resolve_shard(const NeutralHipParticle* particles, int nparticles, Stats* stats, Shard* s) {
  if (stats) {
    memset(stats, 0, sizeof(*stats));
  }
  const State::Store* st = find_store(particles);
  if (st && st->decomposed) {
    return 2;
  }
  s->n = st ? st->count : nparticles;
  s->pid_base = st ? st->first : g.pid_base;
  return (!particles || s->n <= 0) ? 1 : 0;
}

/* The arrays made current (where the call reads the store), the shared workspace grown to `bytes`, launch(workspace) between the two
 * events, and the head of the workspace read into *header with the call's one wait; -> the
 * milliseconds between the events. */
template <class Header, class Launch>
double run_census_op(size_t bytes, Header* header, Launch launch, bool reads_store = true) {
  ensure_scratch();
  if (reads_store) {
    g.mirror.write_back(); /* lazy export, a pending write-back: the arrays are read */
  }
  ensure_capacity(g.census, bytes, bytes);
  HIP_CHECK(hipEventRecord(g.ev_start, g.stream));
  HIP_CHECK(launch(g.census.d));
  HIP_CHECK(hipEventRecord(g.ev_stop, g.stream));
  HIP_CHECK(hipMemcpyAsync(header, g.census.d, sizeof(*header), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  float ms = 0.0f;
  HIP_CHECK(hipEventElapsedTime(&ms, g.ev_start, g.ev_stop));
  return (double)ms;
}

/* ---- ... and what the three sources share beyond that ---- */
bool positive(double v) { return std::isfinite(v) && v > 0.0; }
bool extent(double v) { return std::isfinite(v) && v >= 0.0; }

/* an emission's common arguments: how many, at what weight, over what timestep, into what mesh */
bool emission_ok(int count, double weight, double dt, const double* edgex, const double* edgey, int local_nx,
                 int local_ny, int pad) {
  return count >= 0 && positive(weight) && positive(dt) && edgex && edgey && local_nx >= 1 && local_ny >= 1 &&
         pad >= 0;
}

/* `count` of the caller's bins checked and copied as the fill reads them; *sum: the running sum of
 * their shares, left to right with one addition each -- the fill's walk over the bins repeats these
 * additions bit for bit.  -> false at a bin the call refuses */
bool copy_bins(const NeutralHipSourceBin* bins, int count, neutral::DescribedBin* out, double* sum) {
  for (int b = 0; b < count; ++b) {
    if (!positive(bins[b].share) || !positive(bins[b].e_lo) || !std::isfinite(bins[b].e_hi) ||
        bins[b].e_hi < bins[b].e_lo) {
      return false;
    }
    *sum = b == 0 ? bins[b].share : *sum + bins[b].share;
    out[b] = neutral::DescribedBin{bins[b].e_lo, bins[b].e_hi, bins[b].share};
  }
  return true;
}

/* what every source's stats say of an emission, and the arrays marked where it wrote to them */
template <class Stats>
void emission_done(const neutral::SourceHeader& h, double weight, double ms, const NeutralHipParticle* particles,
                   Stats* stats) {
  if (stats) {
    stats->dead_before = h.dead;
    stats->emitted = h.emitted;
    stats->weight_emitted = (double)h.emitted * weight;
    stats->source_ms = ms;
  }
  if (h.emitted > 0) {
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  }
}

/* what a window that ran says of itself, plain or grouped */
void window_results(const neutral::WindowHeader& h, NeutralHipWindowStats* stats) {
  stats->below = h.killed + h.survived;
  stats->roulette_killed = h.killed;
  stats->roulette_survived = h.survived;
  stats->above = h.above;
  stats->split = h.split;
  stats->copies_made = h.granted;
  stats->copies_refused = h.demand - h.granted;
  stats->roulette_weight_lost = h.lost;
  stats->roulette_weight_gained = h.gained;
}

/* 1 .. kSpectrumMaxGroups groups, every edge finite and > 0, strictly ascending: the spectrum tally's
 * rule, and the grouped census's and window's */
bool group_edges_ok(int ngroups, const double* edges) {
  if (ngroups < 1 || ngroups > neutral::kSpectrumMaxGroups || edges == nullptr) {
    return false;
  }
  for (int i = 0; i <= ngroups; ++i) {
    if (!std::isfinite(edges[i]) || !(edges[i] > 0.0) || (i > 0 && !(edges[i] > edges[i - 1]))) {
      return false;
    }
  }
  return true;
}

/* what the blocks calls take for a mesh: blocks of at least one cell, 0 groups and no edges or
 * valid groups, at most 0x3fffffff bins; *b: the coarse mesh */
bool block_mesh_ok(int nx, int ny, int block_x, int block_y, int ngroups, const double* edges,
                   neutral::BlockMesh* b) {
  if (nx < 1 || ny < 1 || block_x < 1 || block_y < 1) {
    return false;
  }
  if (ngroups == 0 ? edges != nullptr : !group_edges_ok(ngroups, edges)) {
    return false;
  }
  *b = neutral::BlockMesh::of(nx, ny, block_x, block_y);
  return (long long)b->cnx * b->cny * (ngroups > 0 ? ngroups : 1) <= 0x3fffffffll;
}

}  // namespace

extern "C" {

size_t allocate_data(double** buf, size_t len) {
  *buf = (double*)device_zalloc(sizeof(double) * len);
  return sizeof(double) * len;
}
size_t allocate_float_data(float** buf, size_t len) {
  *buf = (float*)device_zalloc(sizeof(float) * len);
  return sizeof(float) * len;
}
size_t allocate_int_data(int** buf, size_t len) {
  *buf = (int*)device_zalloc(sizeof(int) * len);
  return sizeof(int) * len;
}
size_t allocate_uint64_data(uint64_t** buf, size_t len) {
  *buf = (uint64_t*)device_zalloc(sizeof(uint64_t) * len);
  return sizeof(uint64_t) * len;
}
void allocate_host_data(double** buf, size_t len) {
  *buf = (double*)calloc(len ? len : 1, sizeof(double));
  if (!*buf) {
    fprintf(stderr, "Could not allocate host data.\n");
    exit(EXIT_FAILURE);
  }
}
void allocate_host_int_data(int** buf, size_t len) {
  *buf = (int*)calloc(len ? len : 1, sizeof(int));
  if (!*buf) {
    fprintf(stderr, "Could not allocate host data.\n");
    exit(EXIT_FAILURE);
  }
}
void deallocate_data(double* buf) { HIP_CHECK(hipFree(buf)); }
void deallocate_int_data(int* buf) { HIP_CHECK(hipFree(buf)); }
void deallocate_uint64_data(uint64_t* buf) { HIP_CHECK(hipFree(buf)); }
void deallocate_host_data(double* buf) { free(buf); }

void copy_buffer(const size_t len, double** src, double** dst, int send) {
  const hipMemcpyKind kind = send ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
  if (send) {
    if (g.mirror.overlaps(*src, sizeof(double) * len)) g.mirror.write_back(); /* lazy export pending */
  } else {
    before_device_write(*dst, sizeof(double) * len);
  }
  HIP_CHECK(hipMemcpyAsync(*dst, *src, sizeof(double) * len, kind, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void copy_int_buffer(const size_t len, int** src, int** dst, int send) {
  const hipMemcpyKind kind = send ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
  if (send) {
    if (g.mirror.overlaps(*src, sizeof(int) * len)) g.mirror.write_back(); /* lazy export pending */
  } else {
    before_device_write(*dst, sizeof(int) * len);
  }
  HIP_CHECK(hipMemcpyAsync(*dst, *src, sizeof(int) * len, kind, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void move_host_buffer_to_device(const size_t len, double** src, double** dst) {
  HIP_CHECK(hipMalloc((void**)dst, sizeof(double) * (len ? len : 1)));
  HIP_CHECK(hipMemcpyAsync(*dst, *src, sizeof(double) * len, hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  free(*src);
  *src = NULL;
}

/* ---- 3. extensions ------------------------------------------------------------ */

int neutral_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    return 0;
  }
  return n;
}

int neutral_hip_set_device(int device) {
  return hipSetDevice(device) == hipSuccess ? 0 : 1;
}

void neutral_hip_set_stream(void* hip_stream) { g.stream = (hipStream_t)hip_stream; }
void neutral_hip_set_pid_base(uint64_t pid_base) { g.pid_base = pid_base; }
uint64_t neutral_hip_get_pid_base(void) { return g.pid_base; }

int neutral_hip_set_variant(int variant) {
  if (variant != NEUTRAL_HIP_VARIANT_OVER_PARTICLE &&
      variant != NEUTRAL_HIP_VARIANT_EVENT_SORTED && variant != NEUTRAL_HIP_VARIANT_TILED) {
    return 1;
  }
  g.variant = variant;
  g.variant_from_env_done = true; /* an explicit choice overrides the environment */
  return 0;
}

void neutral_hip_set_quiet(int quiet) { g.quiet = quiet; }

int neutral_hip_set_arithmetic(int mode) {
  if (mode != NEUTRAL_HIP_ARITH_AUTO && mode != NEUTRAL_HIP_ARITH_CHECKED) {
    return 1;
  }
  g.arithmetic = mode;
  g.arithmetic_from_env_done = true; /* an explicit choice overrides the environment */
  g.use_checked = false;             /* (auto mode starts over: the next step's check decides) */
  return 0;
}

void neutral_hip_set_tests_file(const char* path) {
  strncpy(g.tests_file, path, NEUTRAL_MAX_STR_LEN - 1);
  g.tests_file[NEUTRAL_MAX_STR_LEN - 1] = '\0';
}

void neutral_hip_last_step(NeutralHipStepStats* stats) { *stats = g.last; }

void neutral_hip_reinject_particles(const int nparticles, const int local_nx,
                                    const int local_ny, const int pad,
                                    const double local_particle_left_off,
                                    const double local_particle_bottom_off,
                                    const double local_particle_width,
                                    const double local_particle_height, const int x_off,
                                    const int y_off, const double dt, const double* edgex,
                                    const double* edgey, const double initial_energy,
                                    NeutralHipParticle* particles) {
  const State::Store* st = find_store(particles);
  if (st && st->decomposed) {
    run_inject_filtered(const_cast<State::Store*>(st), st->capacity, local_nx, local_ny, pad,
                        local_particle_left_off, local_particle_bottom_off, local_particle_width,
                        local_particle_height, x_off, y_off, dt, edgex, edgey, initial_energy,
                        particles);
    return;
  }
  if (st) {
    g.pid_base = st->first; /* this rank's shard, whatever count the caller names */
  }
  run_inject(st ? st->count : nparticles, local_nx, local_ny, pad, local_particle_left_off,
             local_particle_bottom_off, local_particle_width, local_particle_height, x_off,
             y_off, dt, edgex, edgey, initial_energy, particles);
}

void neutral_hip_set_lazy_export(int lazy) { g.lazy_export = lazy; }

void neutral_hip_set_stream_queues(int on) { g.stream_queues = on ? 1 : 0; }

void neutral_hip_sync_particles(NeutralHipParticle* particles) {
  (void)particles; /* at most one store has a pending write-back */
  g.mirror.write_back();
}

void neutral_hip_invalidate_particles(NeutralHipParticle* particles) {
  if (particles && g.mirror.owns(particles)) {
    /* whatever the records hold that the arrays do not have yet goes out first, so
     * a caller that changed SOME particles keeps the others */
    g.mirror.write_back();
    g.mirror.drop();
  }
}

int neutral_hip_comb_particles(NeutralHipParticle* particles, int nparticles, uint64_t seed,
                               NeutralHipCombStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  neutral::CombHeader h;
  const double ms = run_census_op(neutral::comb_workspace_bytes(s.n), &h, [&](void* workspace) {
    return neutral::launch_comb(view_of(particles), s.n, UINT64_MAX - s.pid_base, seed, workspace, g.stream);
  });
  if (stats) {
    stats->live_before = h.live;
    stats->weight_before = h.weight;
    stats->comb_ms = ms;
  }
  if (!h.go) {
    return 1;
  }
  g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  if (stats) {
    stats->sources_kept = h.sources;
    stats->max_copies = h.max_copies;
    stats->weight_each = h.weight_each;
  }
  return 0;
}

int neutral_hip_source_particles(NeutralHipParticle* particles, int nparticles, int count,
                                 double weight, uint64_t seed, const int local_nx,
                                 const int local_ny, const int pad, const double left_off,
                                 const double bottom_off, const double width, const double height,
                                 const int x_off, const int y_off, const double dt,
                                 const double* edgex, const double* edgey,
                                 const double initial_energy, NeutralHipSourceStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  if (!emission_ok(count, weight, dt, edgex, edgey, local_nx, local_ny, pad) || !positive(initial_energy) ||
      !extent(width) || !extent(height)) {
    return 1;
  }
  const double box[4] = {left_off, bottom_off, width, height};
  const neutral::InjectArgs a =
      inject_args(s, particles, local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey, box, initial_energy);
  neutral::SourceHeader h;
  const double ms = run_census_op(neutral::source_workspace_bytes(s.n), &h, [&](void* workspace) {
    return neutral::launch_source(a, s.n, count, weight, seed, workspace, g.stream);
  });
  emission_done(h, weight, ms, particles, stats);
  return 0;
}

int neutral_hip_source_described(NeutralHipParticle* particles, int nparticles, int count,
                                 double weight, uint64_t seed, int ncomponents,
                                 const NeutralHipSourceComponent* components, int nbins,
                                 const NeutralHipSourceBin* bins, const int local_nx,
                                 const int local_ny, const int pad, const int x_off, const int y_off,
                                 const double dt, const double* edgex, const double* edgey,
                                 NeutralHipDescribedSourceStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  if (!emission_ok(count, weight, dt, edgex, edgey, local_nx, local_ny, pad)) {
    return 1;
  }
  if (ncomponents < 1 || ncomponents > neutral::kDescribedMaxComponents || nbins < 1 ||
      nbins > neutral::kDescribedMaxBins || !components || !bins) {
    return 1;
  }
  /* the tables as the fill reads them: every bin, then C_k and S_k beside each component, one
   * addition each */
  neutral::DescribedTables tables;
  memset(&tables, 0, sizeof(tables));
  double in_bins = 0.0;
  if (!copy_bins(bins, nbins, tables.bins, &in_bins)) {
    return 1;
  }
  double running = 0.0;
  for (int k = 0; k < ncomponents; ++k) {
    const NeutralHipSourceComponent& c = components[k];
    if (!positive(c.share) || !std::isfinite(c.left) || !std::isfinite(c.bottom) || !extent(c.width) ||
        !extent(c.height) || !std::isfinite(c.theta0) || !extent(c.theta_width) || c.bin_first < 0 ||
        c.bin_count < 1 || c.bin_first > nbins - c.bin_count) {
      return 1;
    }
    running = k == 0 ? c.share : running + c.share;
    copy_bins(bins + c.bin_first, c.bin_count, tables.bins + c.bin_first, &in_bins); /* (its own sum) */
    if (!std::isfinite(running) || !std::isfinite(in_bins)) {
      return 1; /* (shares that are finite one by one and not in sum) */
    }
    tables.components[k] = neutral::DescribedComponent{c.left,   c.bottom,      c.width, c.height,
                                                       c.theta0, c.theta_width, running, in_bins,
                                                       c.bin_first, c.bin_count};
  }
  const neutral::InjectArgs a = inject_args(s, particles, local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey);
  neutral::DescribedSourceHeader h;
  const double ms = run_census_op(neutral::described_workspace_bytes(s.n), &h, [&](void* workspace) {
    return neutral::launch_described_source(a, s.n, count, weight, seed, &tables, ncomponents, nbins,
                                            workspace, g.stream);
  });
  if (stats) {
    for (int k = 0; k < ncomponents; ++k) {
      stats->emitted_by_component[k] = h.by_component[k];
    }
  }
  emission_done(h.base, weight, ms, particles, stats);
  return 0;
}

int neutral_hip_source_mesh(NeutralHipParticle* particles, int nparticles, int count, double weight,
                            uint64_t seed, const double* strength, double theta0, double theta_width,
                            int nbins, const NeutralHipSourceBin* bins, const int local_nx,
                            const int local_ny, const int pad, const int x_off, const int y_off,
                            const double dt, const double* edgex, const double* edgey,
                            NeutralHipMeshSourceStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  if (!emission_ok(count, weight, dt, edgex, edgey, local_nx, local_ny, pad) ||
      (long long)local_nx * local_ny > neutral::kMeshSourceMaxCells) {
    return 1; /* (no mesh to emit from) */
  }
  if (!strength || !std::isfinite(theta0) || !extent(theta_width) || nbins < 1 ||
      nbins > neutral::kDescribedMaxBins || !bins) {
    return 1;
  }
  /* the bins as the fill reads them, and the last of their running sums */
  neutral::MeshSourceBins table;
  memset(&table, 0, sizeof(table));
  double in_bins = 0.0;
  if (!copy_bins(bins, nbins, table.bins, &in_bins) || !std::isfinite(in_bins)) {
    return 1; /* (the second: shares that are finite one by one and not in sum) */
  }
  const neutral::InjectArgs a = inject_args(s, particles, local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey);
  const neutral::MeshSourceArgs m{strength, theta0, theta_width, in_bins, nbins};
  neutral::MeshSourceHeader h;
  const double ms = run_census_op(
      neutral::mesh_source_workspace_bytes(s.n, (long long)local_nx * local_ny), &h, [&](void* workspace) {
        return neutral::launch_mesh_source(a, s.n, count, weight, seed, m, &table, workspace, g.stream);
      });
  if (stats) {
    stats->dead_before = h.base.dead;
    stats->cells_nonzero = h.nonzero;
    stats->strength_total = h.total;
    stats->source_ms = ms;
  }
  if (!h.go) {
    return 1; /* (found on the device: a strength that is negative or not finite, or no S > 0) */
  }
  emission_done(h.base, weight, ms, particles, stats);
  return 0;
}

int neutral_hip_source_bank(NeutralHipParticle* particles, int nparticles, const NeutralHipEscapeRecord* records,
                            uint64_t first, int count, double weight_scale, const double* shift, double snap,
                            const int local_nx, const int local_ny, const int pad, const int x_off,
                            const int y_off, const double dt, const double* edgex, const double* edgey,
                            NeutralHipBankSourceStats* stats) {
  Shard s;
  const int rc = resolve_shard(particles, nparticles, stats, &s);
  if (stats) {
    stats->first_bad = UINT64_MAX;
  }
  if (rc) {
    return rc;
  }
  if (!emission_ok(count, weight_scale, dt, edgex, edgey, local_nx, local_ny, pad) || !records || !extent(snap)) {
    return 1;
  }
  neutral::BankSourceArgs b = {};
  b.records = (const neutral::EscapeRecord*)records;
  b.first = first;
  b.weight_scale = weight_scale;
  b.snap = snap;
  for (int i = 0; i < 8; ++i) {
    b.shift[i] = shift ? shift[i] : 0.0;
    if (!std::isfinite(b.shift[i])) {
      return 1;
    }
  }
  const neutral::InjectArgs a = inject_args(s, particles, local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey);
  neutral::BankSourceHeader h;
  const double ms = run_census_op(neutral::bank_source_workspace_bytes(s.n), &h, [&](void* workspace) {
    return neutral::launch_bank_source(a, s.n, count, b, workspace, g.stream);
  });
  if (stats) {
    stats->dead_before = h.base.dead;
    stats->first_bad = h.first_bad;
    stats->source_ms = ms;
  }
  if (h.first_bad != UINT64_MAX) {
    return 3; /* (found on the device before anything was written) */
  }
  if (stats) {
    stats->emitted = h.base.emitted;
    stats->snapped = h.snapped;
    stats->weight_emitted = h.weight;
  }
  if (h.base.emitted > 0) {
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  }
  return 0;
}

int neutral_hip_window_particles(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                 const double* lower, double upper_ratio, double survival_ratio,
                                 int max_split, uint64_t seed, NeutralHipWindowStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  if (!lower || nx < 1 || ny < 1 || !std::isfinite(upper_ratio) || !std::isfinite(survival_ratio) ||
      upper_ratio < 2.0 || survival_ratio < 1.0 || survival_ratio > upper_ratio || max_split < 2 ||
      max_split > 64) {
    return 1;
  }
  const neutral::WindowArgs a{lower, nx, ny, upper_ratio, survival_ratio, max_split, s.pid_base, seed};
  neutral::WindowHeader h;
  const double ms = run_census_op(neutral::window_workspace_bytes(s.n), &h, [&](void* workspace) {
    return neutral::launch_window(view_of(particles), s.n, a, workspace, g.stream);
  });
  if (stats) {
    stats->live_before = h.live;
    stats->dead_before = h.dead;
    stats->window_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a live slot outside the mesh, a bad weight or bound: nothing was written) */
  }
  if (stats) {
    window_results(h, stats);
  }
  if (h.killed + h.survived + h.granted > 0) {
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  }
  return 0;
}

int neutral_hip_census_tally(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                             double* device_out, NeutralHipCensusStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    /* (the call is collective: a rank whose shard of a sharded store is empty has nothing of its
     * own to tally, but the others wait for it in the all-reduce: it goes on, with zeros) */
    const State::Store* st = find_store(particles);
    if (!(rc == 1 && st && st->count == 0 && neutral::comm_nranks() > 1)) {
      return rc;
    }
  }
  if (!device_out || nx < 1 || ny < 1 || (long long)nx * ny > 0x3fffffffll) {
    return 1;
  }
  neutral::CensusHeader h;
  const double ms = run_census_op(neutral::census_workspace_bytes(nx, ny), &h, [&](void* workspace) {
    if (hipError_t e = neutral::launch_census_score(view_of(particles), s.n, nx, ny, workspace, g.stream)) {
      return e;
    }
    /* (several ranks sharing the mesh: the two meshes and the flag, summed on the device) */
    neutral::comm_allreduce_sum(neutral::census_mesh(workspace), neutral::census_mesh_doubles(nx, ny), true,
                                g.stream);
    return neutral::launch_census_finish(nx, ny, device_out, workspace, g.stream);
  });
  if (stats) {
    stats->live = h.live;
    stats->dead = h.dead;
    stats->census_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a live slot outside the mesh or a bad weight, on some rank: device_out holds zeros) */
  }
  if (stats) {
    stats->occupied_cells = h.occupied;
    stats->max_count = h.max_count;
    stats->weight = h.weight;
    stats->max_cell_weight = h.max_cell_weight;
  }
  return 0; /* (nothing was written to the store: a tiled store's records stay valid) */
}

int neutral_hip_window_bounds(int nx, int ny, const double* census, double target_population,
                              double upper_ratio, double floor_ratio, int min_count, double* lower_out,
                              NeutralHipBoundsStats* stats) {
  if (stats) {
    memset(stats, 0, sizeof(*stats));
  }
  if (!census || !lower_out || nx < 1 || ny < 1 || (long long)nx * ny > 0x3fffffffll ||
      !std::isfinite(target_population) || !std::isfinite(upper_ratio) || !(target_population > 0.0) ||
      upper_ratio < 2.0 || !(floor_ratio >= 0.0) || !(floor_ratio <= 1.0) || min_count < 1) {
    return 1;
  }
  const neutral::BoundsArgs a{census, nx, ny, target_population, upper_ratio, floor_ratio, min_count};
  neutral::BoundsHeader h;
  const double ms = run_census_op(
      neutral::census_workspace_bytes(nx, ny), &h,
      [&](void* workspace) { return neutral::launch_bounds(a, lower_out, workspace, g.stream); },
      /*reads_store=*/false);
  if (stats) {
    stats->bounds_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a census entry negative or not finite, or no eligible cell: lower_out is untouched) */
  }
  if (stats) {
    stats->windowed_cells = h.eligible;
    stats->floored_cells = h.floored;
    stats->max_cell_weight = h.max_cell_weight;
    stats->lower_at_peak = h.peak;
  }
  return 0;
}

int neutral_hip_census_tally_groups(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                    int ngroups, const double* edges, double* device_out,
                                    NeutralHipGroupCensusStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    /* (collective, as the plain census: a rank with an empty shard takes part with zeros) */
    const State::Store* st = find_store(particles);
    if (!(rc == 1 && st && st->count == 0 && neutral::comm_nranks() > 1)) {
      return rc;
    }
  }
  if (!device_out || nx < 1 || ny < 1 || !group_edges_ok(ngroups, edges) ||
      (long long)nx * ny * ngroups > 0x3fffffffll) {
    return 1;
  }
  const int rows = ngroups * ny; /* G meshes back to back: one of nx by G * ny */
  neutral::GroupCensusHeader h;
  const double ms =
      run_census_op(neutral::census_groups_workspace_bytes(nx, ny, ngroups), &h, [&](void* workspace) {
        if (hipError_t e = neutral::launch_census_score_groups(view_of(particles), s.n, nx, ny, ngroups, edges,
                                                               workspace, g.stream)) {
          return e;
        }
        /* (several ranks sharing the mesh: the 2 * G * nx * ny bins and the flag, summed on the device) */
        neutral::comm_allreduce_sum(neutral::census_mesh(workspace), neutral::census_mesh_doubles(nx, rows),
                                    true, g.stream);
        return neutral::launch_census_finish(nx, rows, device_out, workspace, g.stream);
      });
  if (stats) {
    stats->live = h.census.live;
    stats->dead = h.census.dead;
    stats->census_ms = ms;
  }
  if (!h.census.go) {
    return 1; /* (a live slot outside the mesh or a bad weight, on some rank: device_out holds zeros) */
  }
  if (stats) {
    stats->outside = h.outside;
    stats->occupied_bins = h.census.occupied;
    stats->max_count = h.census.max_count;
    stats->weight = h.census.weight;
    stats->max_bin_weight = h.census.max_cell_weight;
  }
  return 0; /* (nothing was written to the store: a tiled store's records stay valid) */
}

int neutral_hip_window_particles_groups(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                        int ngroups, const double* edges, const double* lower,
                                        double upper_ratio, double survival_ratio, int max_split,
                                        uint64_t seed, NeutralHipGroupWindowStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  if (!lower || nx < 1 || ny < 1 || !std::isfinite(upper_ratio) || !std::isfinite(survival_ratio) ||
      upper_ratio < 2.0 || survival_ratio < 1.0 || survival_ratio > upper_ratio || max_split < 2 ||
      max_split > 64 || !group_edges_ok(ngroups, edges) || (long long)nx * ny * ngroups > 0x3fffffffll) {
    return 1;
  }
  const neutral::WindowArgs a{lower, nx, ny, upper_ratio, survival_ratio, max_split, s.pid_base, seed};
  neutral::GroupWindowHeader gh;
  const double ms = run_census_op(neutral::window_groups_workspace_bytes(s.n), &gh, [&](void* workspace) {
    return neutral::launch_window_groups(view_of(particles), s.n, a, ngroups, edges, workspace, g.stream);
  });
  const neutral::WindowHeader& h = gh.window;
  if (stats) {
    stats->window.live_before = h.live;
    stats->window.dead_before = h.dead;
    stats->window.window_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a live slot outside the mesh, a bad weight or bound: nothing was written) */
  }
  if (stats) {
    window_results(h, &stats->window);
    stats->outside = gh.outside;
  }
  if (h.killed + h.survived + h.granted > 0) {
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  }
  return 0;
}

int neutral_hip_census_tally_blocks(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                    int block_x, int block_y, int ngroups, const double* edges,
                                    double* device_out, NeutralHipBlockCensusStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    /* (collective, as the plain census: a rank with an empty shard takes part with zeros) */
    const State::Store* st = find_store(particles);
    if (!(rc == 1 && st && st->count == 0 && neutral::comm_nranks() > 1)) {
      return rc;
    }
  }
  neutral::BlockMesh b;
  if (!device_out || !block_mesh_ok(nx, ny, block_x, block_y, ngroups, edges, &b)) {
    return 1;
  }
  if (!g.tuning_read) { /* (the CU count, read once) */
    g.tuning = neutral::launch_tuning_from_env();
    g.tuning_read = true;
  }
  /* NEUTRAL_CENSUS_LDS_BINS: the most bins the pass keeps in LDS (0: never), read per call -- the
   * A/B of the two forms and the tests set it between calls */
  int lds_max_bins = neutral::kCensusLdsBins;
  if (const char* v = getenv("NEUTRAL_CENSUS_LDS_BINS")) {
    char* end = nullptr;
    const long asked = strtol(v, &end, 10);
    if (end != v && asked >= 0) {
      lds_max_bins = asked < neutral::kCensusLdsBinsMax ? (int)asked : neutral::kCensusLdsBinsMax;
    }
  }
  const int meshes = ngroups > 0 ? ngroups : 1;
  const int rows = meshes * b.cny; /* max(G, 1) coarse meshes back to back: one of cnx by rows */
  bool privatised = false;
  neutral::GroupCensusHeader h;
  const double ms =
      run_census_op(neutral::census_groups_workspace_bytes(b.cnx, b.cny, meshes), &h, [&](void* workspace) {
        if (hipError_t e = neutral::launch_census_score_blocks(view_of(particles), s.n, nx, ny, b, ngroups, edges,
                                                               lds_max_bins, g.tuning.compute_units, workspace,
                                                               g.stream, &privatised)) {
          return e;
        }
        /* (several ranks sharing the mesh: the 2 * B bins and the flag, summed on the device) */
        neutral::comm_allreduce_sum(neutral::census_mesh(workspace), neutral::census_mesh_doubles(b.cnx, rows),
                                    true, g.stream);
        return neutral::launch_census_finish(b.cnx, rows, device_out, workspace, g.stream);
      });
  if (stats) {
    stats->census.live = h.census.live;
    stats->census.dead = h.census.dead;
    stats->census.census_ms = ms;
    stats->privatised = privatised ? 1u : 0u;
  }
  if (!h.census.go) {
    return 1; /* (a live slot off the true mesh or a bad weight, on some rank: device_out holds zeros) */
  }
  if (stats) {
    stats->census.outside = h.outside;
    stats->census.occupied_bins = h.census.occupied;
    stats->census.max_count = h.census.max_count;
    stats->census.weight = h.census.weight;
    stats->census.max_bin_weight = h.census.max_cell_weight;
  }
  return 0; /* (nothing was written to the store: a tiled store's records stay valid) */
}

int neutral_hip_window_particles_blocks(NeutralHipParticle* particles, int nparticles, int nx, int ny,
                                        int block_x, int block_y, int ngroups, const double* edges,
                                        const double* lower, double upper_ratio, double survival_ratio,
                                        int max_split, uint64_t seed, NeutralHipGroupWindowStats* stats) {
  Shard s;
  if (const int rc = resolve_shard(particles, nparticles, stats, &s)) {
    return rc;
  }
  neutral::BlockMesh b;
  if (!lower || !std::isfinite(upper_ratio) || !std::isfinite(survival_ratio) || upper_ratio < 2.0 ||
      survival_ratio < 1.0 || survival_ratio > upper_ratio || max_split < 2 || max_split > 64 ||
      !block_mesh_ok(nx, ny, block_x, block_y, ngroups, edges, &b)) {
    return 1;
  }
  const neutral::WindowArgs a{lower, nx, ny, upper_ratio, survival_ratio, max_split, s.pid_base, seed};
  neutral::GroupWindowHeader gh;
  const double ms = run_census_op(neutral::window_groups_workspace_bytes(s.n), &gh, [&](void* workspace) {
    return neutral::launch_window_blocks(view_of(particles), s.n, a, b, ngroups, edges, workspace, g.stream);
  });
  const neutral::WindowHeader& h = gh.window;
  if (stats) {
    stats->window.live_before = h.live;
    stats->window.dead_before = h.dead;
    stats->window.window_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a live slot off the true mesh, a bad weight or bound: nothing was written) */
  }
  if (stats) {
    window_results(h, &stats->window);
    stats->outside = gh.outside;
  }
  if (h.killed + h.survived + h.granted > 0) {
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false);
  }
  return 0;
}

int neutral_hip_batch_fold(const double* x, size_t len, int k, double* moments,
                           NeutralHipBatchFoldStats* stats) {
  if (stats) {
    memset(stats, 0, sizeof(*stats));
  }
  if (!x || !moments || len < 1 || len > ((size_t)1 << 30) || k < 1) {
    return 1;
  }
  neutral::BatchHeader h;
  const double ms = run_census_op(
      neutral::batch_workspace_bytes(len), &h,
      [&](void* workspace) { return neutral::launch_batch_fold(x, len, k, moments, workspace, g.stream); },
      /*reads_store=*/false);
  if (stats) {
    stats->fold_ms = ms;
  }
  if (!h.go) {
    return 1; /* (an entry of x is not finite: moments is untouched) */
  }
  if (stats) {
    stats->sum = h.sum;
    stats->nonzero = h.nonzero;
  }
  return 0;
}

int neutral_hip_batch_statistics(const double* moments, size_t len, int nbatches, double scale,
                                 double* estimate_out, double* relerr_out, NeutralHipBatchStats* stats) {
  if (stats) {
    memset(stats, 0, sizeof(*stats));
  }
  if (!moments || !estimate_out || !relerr_out || len < 1 || len > ((size_t)1 << 30) || nbatches < 2 ||
      !std::isfinite(scale) || !(scale > 0.0)) {
    return 1;
  }
  neutral::BatchHeader h;
  const double ms = run_census_op(
      neutral::batch_workspace_bytes(len), &h,
      [&](void* workspace) {
        return neutral::launch_batch_statistics(moments, len, nbatches, scale, estimate_out, relerr_out,
                                                workspace, g.stream);
      },
      /*reads_store=*/false);
  if (stats) {
    stats->stats_ms = ms;
  }
  if (!h.go) {
    return 1; /* (a mean not finite, an M2 negative or not finite: both outputs are untouched) */
  }
  if (stats) {
    stats->scored = h.scored;
    stats->within_10pc = h.within10;
    stats->within_5pc = h.within5;
    stats->max_relerr = h.max_relerr;
    stats->mean_relerr = h.mean_relerr;
    stats->estimate_sum = h.sum;
  }
  return 0;
}

void neutral_hip_set_scalar_flux_tally(double* device_tally) { g.tallies[kTallyFlux].caller[0] = device_tally; }

int neutral_hip_set_roulette(double weight_cutoff, double survival_weight) {
  const bool finite = std::isfinite(weight_cutoff) && std::isfinite(survival_weight);
  if (!finite || weight_cutoff < 0.0 || survival_weight < 0.0 ||
      (weight_cutoff == 0.0) != (survival_weight == 0.0) || survival_weight < weight_cutoff) {
    return 1; /* refused: the setting stays as it was */
  }
  if (weight_cutoff > 0.0 && g.window_roulette.lower) {
    return 1; /* (the two roulettes are exclusive: neutral_hip_set_window_roulette) */
  }
  g.roulette_cutoff = weight_cutoff;
  g.roulette_survival = survival_weight;
  return 0;
}

int neutral_hip_set_window_roulette(int nx, int ny, const double* lower, double survival_ratio, int ngroups,
                                    const double* edges, int block_x, int block_y) {
  if (lower == nullptr) {
    g.window_roulette.lower = nullptr; /* off */
    return 0;
  }
  neutral::BlockMesh b;
  if (!std::isfinite(survival_ratio) || survival_ratio < 1.0 || !block_mesh_ok(nx, ny, block_x, block_y, ngroups, edges, &b) ||
      g.roulette_cutoff > 0.0) {
    return 1; /* refused: the setting stays as it was */
  }
  /* the mesh as it stands now: no entry negative or not finite */
  const long long bins = (long long)b.cnx * b.cny * (ngroups > 0 ? ngroups : 1);
  neutral::MeshCheckHeader h;
  run_census_op(
      sizeof(h), &h, [&](void* workspace) { return neutral::launch_window_mesh_check(lower, bins, workspace, g.stream); },
      /*reads_store=*/false);
  if (h.bad != 0) {
    return 1;
  }
  neutral::WindowRouletteParams& w = g.window_roulette;
  w.lower = lower;
  w.survival_ratio = survival_ratio;
  w.nx = nx;
  w.ny = ny;
  w.cnx = b.cnx;
  w.cny = b.cny;
  w.blocks = (block_x != 1 || block_y != 1) ? 1 : 0;
  w.ngroups = ngroups;
  w.by_x = neutral::BlockDivisor::of(block_x);
  w.by_y = neutral::BlockDivisor::of(block_y);
  for (int i = 0; i <= ngroups && ngroups > 0; ++i) {
    w.edges[i] = edges[i];
  }
  return 0;
}

int neutral_hip_set_spectrum_tally(int ngroups, const double* edges, int x0, int y0, int x1, int y1,
                                   double* device_out) {
  if (device_out == nullptr) {
    g.spectrum_out = nullptr; /* off */
    return 0;
  }
  if (!group_edges_ok(ngroups, edges)) {
    return 1; /* refused: the setting stays as it was */
  }
  /* (the mesh is not known here: a box that reaches beyond it covers the cells it contains) */
  if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0) {
    return 1;
  }
  g.spectrum_out = device_out;
  g.spectrum_ngroups = ngroups;
  for (int i = 0; i <= ngroups; ++i) {
    g.spectrum_edges[i] = edges[i];
  }
  g.spectrum_box[0] = x0;
  g.spectrum_box[1] = y0;
  g.spectrum_box[2] = x1;
  g.spectrum_box[3] = y1;
  return 0;
}

int neutral_hip_set_collision_tallies(double* collisions, double* absorbed) {
  if ((collisions == nullptr) != (absorbed == nullptr)) {
    return 1; /* one without the other: refused, the setting stays as it was */
  }
  g.tallies[kTallyCollisions].caller[0] = collisions;
  g.tallies[kTallyCollisions].caller[1] = absorbed;
  return 0;
}

int neutral_hip_set_current_tally(double* jx, double* jy) {
  if ((jx == nullptr) != (jy == nullptr)) {
    return 1; /* one without the other: refused, the setting stays as it was */
  }
  g.tallies[kTallyCurrent].caller[0] = jx;
  g.tallies[kTallyCurrent].caller[1] = jy;
  return 0;
}

void neutral_hip_set_outflow_tally(double* device_out) { g.tallies[kTallyOutflow].caller[0] = device_out; }

/* the outer sides of the axes in a periodic mask, as the vacuum mask numbers them */
static unsigned periodic_sides(unsigned axes) { return ((axes & 1u) ? 3u : 0u) | ((axes & 2u) ? 12u : 0u); }

int neutral_hip_set_vacuum_sides(unsigned sides) {
  if (sides > 15u) {
    return 1; /* a bit above 8: refused, the setting stays as it was */
  }
  if ((sides & periodic_sides(g.periodic_axes)) != 0u) {
    return 1; /* a side of an axis that is periodic: likewise */
  }
  g.vacuum_sides = sides;
  return 0;
}

unsigned neutral_hip_get_vacuum_sides(void) { return g.vacuum_sides; }

int neutral_hip_set_periodic_axes(unsigned axes) {
  if (axes > 3u) {
    return 1; /* a bit above 2: refused, the setting stays as it was */
  }
  if ((g.vacuum_sides & periodic_sides(axes)) != 0u) {
    return 1; /* a side of a requested axis is vacuum: likewise */
  }
  g.periodic_axes = axes;
  return 0;
}

unsigned neutral_hip_get_periodic_axes(void) { return g.periodic_axes; }

void neutral_hip_last_wraps(NeutralHipWrapStats* out) {
  if (out) {
    *out = g.last_wraps;
  }
}

int neutral_hip_set_leakage_tally(int ngroups, const double* edges, int ncosines, double* device_out) {
  if (device_out == nullptr) {
    g.leakage_out = nullptr; /* off */
    return 0;
  }
  if (ncosines < 1 || ncosines > neutral::kLeakageMaxCosines ||
      (ngroups == 0 ? edges != nullptr : !group_edges_ok(ngroups, edges))) {
    return 1; /* refused: the setting stays as it was */
  }
  g.leakage_out = device_out;
  g.leakage_ngroups = ngroups;
  g.leakage_ncosines = ncosines;
  for (int i = 0; i <= ngroups && ngroups > 0; ++i) {
    g.leakage_edges[i] = edges[i];
  }
  g.leakage_edges_uploaded = false; /* (the next step that scores copies them to the device) */
  return 0;
}

static_assert(sizeof(NeutralHipEscapeRecord) == sizeof(neutral::EscapeRecord) &&
                  offsetof(NeutralHipEscapeRecord, time_left) == offsetof(neutral::EscapeRecord, time_left) &&
                  offsetof(NeutralHipEscapeRecord, slot) == offsetof(neutral::EscapeRecord, slot) &&
                  offsetof(NeutralHipEscapeRecord, side) == offsetof(neutral::EscapeRecord, side),
              "the kernels' escape record is the interface's");

int neutral_hip_set_escape_bank(NeutralHipEscapeRecord* device_records, uint64_t capacity) {
  if (device_records == nullptr) {
    g.bank_records = nullptr; /* off */
    g.bank_capacity = 0;
    return 0;
  }
  if (capacity == 0 || ((uintptr_t)device_records & 15u) != 0) {
    return 1; /* refused: the setting stays as it was */
  }
  g.bank_records = device_records;
  g.bank_capacity = capacity;
  g.bank_claimed = 0;
  g.bank_step_claimed = g.bank_step_recorded = 0;
  g.bank_zero_pending = true; /* (the next step that records zeroes the cursor on its stream) */
  return 0;
}

int neutral_hip_reset_escape_bank(void) {
  if (g.bank_records == nullptr) {
    return 1;
  }
  g.bank_claimed = 0;
  g.bank_zero_pending = true;
  return 0;
}

void neutral_hip_escape_bank_stats(NeutralHipEscapeBankStats* out) {
  if (out) {
    *out = NeutralHipEscapeBankStats{g.bank_capacity, g.bank_claimed, g.bank_recorded(), g.bank_step_claimed,
                                     g.bank_step_recorded};
  }
}

void neutral_hip_last_escape(NeutralHipEscapeStats* out) {
  if (out) {
    *out = g.last_escape;
  }
}

void neutral_hip_set_auto_shard(int on) { g.auto_shard = on ? 1 : 0; }

int neutral_hip_set_decomposition(int ranks_x, int ranks_y, int global_nx, int global_ny,
                                  int* x_off, int* y_off, int* local_nx, int* local_ny) {
  const int n = neutral::comm_nranks();
  if (ranks_x < 1 || ranks_y < 1 || ranks_x * ranks_y != n || n > 64 ||
      ranks_x > global_nx || ranks_y > global_ny) {
    return 1;
  }
  g.domain.px = ranks_x;
  g.domain.py = ranks_y;
  g.domain.bx = (global_nx + ranks_x - 1) / ranks_x;
  g.domain.by = (global_ny + ranks_y - 1) / ranks_y;
  /* (every rank must own at least one column and one row of cells) */
  if (g.domain.bx * (ranks_x - 1) >= global_nx || g.domain.by * (ranks_y - 1) >= global_ny) {
    return 1;
  }
  g.domain_on = true;
  const int r = neutral::comm_rank();
  const int rx = r % ranks_x;
  const int ry = r / ranks_x;
  *x_off = rx * g.domain.bx;
  *y_off = ry * g.domain.by;
  *local_nx = (rx == ranks_x - 1) ? global_nx - *x_off : g.domain.bx;
  *local_ny = (ry == ranks_y - 1) ? global_ny - *y_off : g.domain.by;
  return 0;
}

void neutral_hip_clear_decomposition(void) {
  g.domain_on = false;
  g.domain = neutral::DomainGrid{1, 1, 0, 0};
  g.source_box_set = false;
}

void neutral_hip_set_source_box(double left, double bottom, double width, double height) {
  g.source_box[0] = left;
  g.source_box[1] = bottom;
  g.source_box[2] = width;
  g.source_box[3] = height;
  g.source_box_set = true;
}

const unsigned* neutral_hip_store_keys(const NeutralHipParticle* particles) {
  const State::Store* st = find_store(particles);
  if (st && st->decomposed && g.mirror.owns(particles)) {
    g.mirror.write_back(); /* (lazy export: the keys move with the arrays) */
  }
  return (st && st->decomposed) ? st->keys : nullptr;
}

int neutral_hip_store_count(const NeutralHipParticle* particles) {
  const State::Store* st = find_store(particles);
  return st ? st->count : -1;
}

void neutral_hip_free_particles(NeutralHipParticle* p) {
  if (!p) {
    return;
  }
  forget_store(p);
  g.mirror.forget(p); /* pending state dies with the store */
  void* arrays[] = {p->x,      p->y,           p->omega_x,          p->omega_y, p->energy,
                    p->weight, p->dt_to_census, p->mfp_to_collision, p->cellx,   p->celly,
                    p->dead};
  for (void* a : arrays) {
    if (a) {
      HIP_CHECK(hipFree(a));
    }
  }
  if (g.census.d) { /* (the workspace of comb, source and window is sized for a store: it goes with one) */
    HIP_CHECK(hipFree(g.census.d));
    g.census = {};
  }
  free(p);
}

void neutral_hip_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes) {
  if (g.mirror.overlaps(src_device, bytes)) g.mirror.write_back(); /* lazy export pending */
  HIP_CHECK(hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void neutral_hip_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes) {
  before_device_write(dst_device, bytes);
  HIP_CHECK(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}
void neutral_hip_memset(void* dst_device, int value, size_t bytes) {
  before_device_write(dst_device, bytes);
  HIP_CHECK(hipMemsetAsync(dst_device, value, bytes, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
}

}  // extern "C"

/* probes: host arrays in, host arrays out; staging through HBM inside */
namespace {
template <typename T>
T* stage_in(const T* host, size_t n) {
  T* d = nullptr;
  HIP_CHECK(hipMalloc((void**)&d, sizeof(T) * (n ? n : 1)));
  if (host && n) {
    HIP_CHECK(hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, g.stream));
  }
  return d;
}
template <typename T>
void stage_out(T* host, T* dev, size_t n) {
  HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));
  HIP_CHECK(hipFree(dev));
}
}  // namespace

extern "C" {

void neutral_hip_probe_threefry(const uint64_t* in3, uint64_t* out2, double* rn2, int n) {
  uint64_t* d_in = stage_in(in3, (size_t)3 * n);
  uint64_t* d_out = stage_in((const uint64_t*)nullptr, (size_t)2 * n);
  double* d_rn = stage_in((const double*)nullptr, (size_t)2 * n);
  HIP_CHECK(neutral::launch_probe_threefry(d_in, d_out, d_rn, n, g.stream));
  stage_out(out2, d_out, (size_t)2 * n);
  stage_out(rn2, d_rn, (size_t)2 * n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_cs_lookup(const NeutralHipCrossSection* cs, const double* energy,
                                 double* value, int* index, int n, int use_index) {
  double* d_e = stage_in(energy, (size_t)n);
  double* d_v = stage_in((const double*)nullptr, (size_t)n);
  int* d_i = stage_in((const int*)nullptr, (size_t)n);
  ensure_scratch();
  neutral::CsIndex ix = {nullptr, 0, 0, 0};
  if (use_index) {
    ix = build_index(cs->keys, cs->nentries, g.d_index[0]);
  }
  HIP_CHECK(neutral::launch_probe_cs(cs->keys, cs->values, cs->nentries, d_e, d_v, d_i, n, ix,
                                     g.stream));
  stage_out(value, d_v, (size_t)n);
  stage_out(index, d_i, (size_t)n);
  HIP_CHECK(hipFree(d_e));
}

void neutral_hip_probe_distance_to_facet(const double* in9, double* distance, int* x_facet,
                                         int n) {
  double* d_in = stage_in(in9, (size_t)9 * n);
  double* d_d = stage_in((const double*)nullptr, (size_t)n);
  int* d_x = stage_in((const int*)nullptr, (size_t)n);
  HIP_CHECK(neutral::launch_probe_facet(d_in, d_d, d_x, n, g.stream));
  stage_out(distance, d_d, (size_t)n);
  stage_out(x_facet, d_x, (size_t)n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_division(const double* in2, double* out2, int* plain, int n) {
  double* d_in = stage_in(in2, (size_t)2 * n);
  double* d_out = stage_in((const double*)nullptr, (size_t)2 * n);
  int* d_p = stage_in((const int*)nullptr, (size_t)n);
  HIP_CHECK(neutral::launch_probe_division(d_in, d_out, d_p, n, g.stream));
  stage_out(out2, d_out, (size_t)2 * n);
  stage_out(plain, d_p, (size_t)n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_log(const double* x, double* out8, int n) {
  double* d_in = stage_in(x, (size_t)n);
  double* d_out = stage_in((const double*)nullptr, (size_t)8 * n);
  HIP_CHECK(neutral::launch_probe_log(d_in, d_out, n, g.stream));
  stage_out(out8, d_out, (size_t)8 * n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_scatter(const double* in4, double* out10, int n) {
  double* d_in = stage_in(in4, (size_t)4 * n);
  double* d_out = stage_in((const double*)nullptr, (size_t)10 * n);
  HIP_CHECK(neutral::launch_probe_scatter(d_in, d_out, n, g.stream));
  stage_out(out10, d_out, (size_t)10 * n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_policy_quotient(const double* in2, double* out8, int n) {
  double* d_in = stage_in(in2, (size_t)2 * n);
  double* d_out = stage_in((const double*)nullptr, (size_t)8 * n);
  HIP_CHECK(neutral::launch_probe_policy_quotient(d_in, d_out, n, g.stream));
  stage_out(out8, d_out, (size_t)8 * n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_probe_policy_root(const double* in2, double* out10, int n) {
  double* d_in = stage_in(in2, (size_t)2 * n);
  double* d_out = stage_in((const double*)nullptr, (size_t)10 * n);
  HIP_CHECK(neutral::launch_probe_policy_root(d_in, d_out, n, g.stream));
  stage_out(out10, d_out, (size_t)10 * n);
  HIP_CHECK(hipFree(d_in));
}

void neutral_hip_synchronize(void) { HIP_CHECK(hipStreamSynchronize(g.stream)); }
int neutral_hip_abi_version(void) { return NEUTRAL_ABI_VERSION; }

}  // extern "C"
