/*
 * neutral_abi.hip -- the C ABI of libneutral_hip.so (include/neutral_hip.h):
 * the three functions of the reference's neutral_interface.h, the HBM flavour
 * of the allocation hooks, and the extension entry points.  Host code only;
 * kernels live in neutral_kernels.hip.
 */
#include "neutral_abi_state.h"

#include <utility>

using namespace neutral_abi;

/* ---- 0. one timestep, phase by phase (solve_transport_2d below is their sequence) ---- */

namespace {

/* HIP-event times of the step's stages, ACCUMULATED over every batch of launches the
 * step needs (the first enqueue, more stream passes when the step outruns the plan,
 * the rounds of a decomposed mesh): each batch brackets itself with the same events
 * and is harvested after the wait that follows it. */
struct StageMs {
  double kernel = 0.0, sort = 0.0, stream = 0.0, collide = 0.0, exported = 0.0, exchange = 0.0;
};

/* One call of solve_transport_2d: what its phases share. */
struct Step {
  neutral::SolveArgs a = {};
  neutral::StepOptions options;
  bool tiled = false;
  bool decomposed = false;
  bool exchange = false;    /* several ranks share the mesh: every batch ends in the tally exchange
                               (a decomposed mesh has nothing to sum: every rank tallies its own cells) */
  bool pass_export = false; /* the SoA arrays are current when the call returns */
  bool checked = false;     /* arithmetic policy of this step's kernels (neutral_device.h) */
  /* several ranks: the store holds this rank's shard (inject_particles made it so), or
   * -- decomposed mesh -- the particles that are inside this rank's block right now */
  State::Store* shard = nullptr;
  /* what the last wait returned */
  neutral::StepCounters hc[2] = {};
  unsigned long long check[8] = {0};
  unsigned ctrl[16] = {0};
  unsigned long long words[kStepWords] = {0}; /* several ranks: the global step words */
  int passes = 0;
  int attempts = 0;
  int same = 0;
  unsigned long long queue_total = 0; /* histories the batches' collision stages were handed */
  uint64_t local_nprocessed = 0; /* (this rank's own, before the ranks' counters are summed) */
  StageMs stage;
};

/* What one batch of launches differs in from another.  (Whether its tallies are exchanged
 * between ranks or added locally, and whether the by-id write-back runs, follow from the
 * step: Step::exchange, Step::pass_export, Step::decomposed.) */
struct BatchSpec {
  neutral::TiledPlan plan;
  int first_pass;
  bool first_sort_timed; /* pass 0's sort is bracketed by an event of its own (later sorts sit
                            inside the stream passes they serve) */
  bool guarded;          /* the kernels may have returned at entry (an attempt the device turns
                            down): the write-back honours the abort flag too, and the check words
                            are read with the results */
  const neutral::SplitExport* split; /* the write-back in two parts, or null */
};

/* The first batch of an attempt.  Stream passes are enqueued on what the last step needed
 * (plus one, which finds nothing to do when the guess holds) without waiting in between;
 * the first step of a problem starts with two. */
BatchSpec first_batch(const neutral::SplitExport* split) {
  BatchSpec spec = {};
  spec.plan.stream_passes = g.mirror.planned_passes() > 0 ? g.mirror.planned_passes() + 1 : 2;
  spec.plan.blocks_per_cu = -1; /* the collision stage sizes itself from its queue */
  spec.first_pass = 0;
  spec.first_sort_timed = true;
  spec.guarded = true;
  spec.split = split;
  return spec;
}

/* ... and one that goes on with the step from pass number first_pass */
BatchSpec later_batch(int stream_passes, int first_pass) {
  BatchSpec spec = {};
  spec.plan.stream_passes = stream_passes;
  spec.plan.blocks_per_cu = -1;
  spec.first_pass = first_pass;
  return spec;
}

void harvest(Step& s, bool with_sort) {
  StageMs& stage = s.stage;
  float ms = 0.0f;
  HIP_CHECK(hipEventElapsedTime(&ms, g.ev_start, g.ev_stop));
  stage.kernel += (double)ms;
  if (s.tiled) {
    if (with_sort) {
      HIP_CHECK(hipEventElapsedTime(&ms, g.ev_start, g.ev_sorted));
      stage.sort += (double)ms;
      HIP_CHECK(hipEventElapsedTime(&ms, g.ev_sorted, g.ev_streamed));
    } else { /* (later sorts sit inside the stream passes they serve) */
      HIP_CHECK(hipEventElapsedTime(&ms, g.ev_start, g.ev_streamed));
    }
    stage.stream += (double)ms;
    HIP_CHECK(hipEventElapsedTime(&ms, g.ev_streamed, g.ev_collected));
    stage.sort += (double)ms; /* (the collision queue's build) */
    HIP_CHECK(hipEventElapsedTime(&ms, g.ev_collected, g.ev_stop));
    stage.collide += (double)ms;
  } else {
    stage.collide += (double)ms;
  }
  HIP_CHECK(hipEventElapsedTime(&ms, g.ev_stop, g.ev_exported));
  stage.exported += (double)ms;
  if (s.exchange) {
    HIP_CHECK(hipEventElapsedTime(&ms, g.ev_exchange_begins, g.ev_exchanged));
    stage.exchange += (double)ms;
  }
}

/* this step's records (t.rec_out until they are rolled) to the SoA arrays, by id */
void export_records_by_id(const Step& s, const int* abort_flag) {
  const neutral::SolveArgs& a = s.a;
  HIP_CHECK(neutral::launch_export_records(
      g.tiled.rec_out, g.tiled.slot_of_id, a.p, a.nparticles, g.stream, abort_flag,
      a.export_skip_long_dead ? neutral::tiled_first_inactive(g.tiled) : nullptr, 0xFFFFFFFFu,
      nullptr, 0, a.export_skip_long_dead != 0));
}

/* One batch of launches and the wait that ends it: the step's kernels, its tallies on their
 * way to the caller, the write-back, the results. */
void run_batch(Step& s, const BatchSpec& spec) {
  neutral::SolveArgs& a = s.a;
  HIP_CHECK(hipEventRecord(g.ev_start, g.stream));
  if (s.tiled) {
    HIP_CHECK(neutral::launch_solve_tiled(a, s.options, g.tiled, g.stream, spec.plan, spec.first_pass,
                                          spec.first_sort_timed ? g.ev_sorted : nullptr, g.ev_streamed,
                                          g.ev_collected, &s.passes, spec.split));
  } else {
    HIP_CHECK(neutral::launch_solve(a, s.options, g.variant, g.stream));
  }
  HIP_CHECK(hipEventRecord(g.ev_stop, g.stream));
  if (s.exchange) {
    exchange_step(a, s.tiled); /* (beside the write-back below) */
  } else {
    tallies_to_caller(a);
  }
  if (spec.split) {
    /* (the pass beside the collision stage: the caller's stream goes on when it is through) */
    HIP_CHECK(neutral::launch_split_export(a, g.tiled, *spec.split, g.ev_collected));
    HIP_CHECK(hipStreamWaitEvent(g.stream, g.ev_split_done, 0));
  } else if (s.pass_export && !s.decomposed) {
    export_records_by_id(s, spec.guarded ? a.abort_flag : nullptr);
  }
  HIP_CHECK(hipEventRecord(g.ev_exported, g.stream));
  /* (whatever else this step enqueues -- more passes for a step that outran its plan -- is
   * followed by the one pass over everybody) */
  a.export_view = nullptr;
  g.tiled.mark_suspended = 0;

  if (s.exchange) {
    finish_exchange();
  }
  /* the one wait of a steady-state step: counters, the pipeline's control words, the
   * verdict on the table view and -- several ranks -- the step words, published by one
   * small kernel into pinned host memory */
  publish_results(s.tiled, s.exchange);
  wait_for_stream();
  fetch_results(s.hc, spec.guarded ? s.check : nullptr, s.tiled ? s.ctrl : nullptr,
                s.exchange ? s.words : nullptr);
  harvest(s, spec.first_sort_timed);
  s.queue_total += s.exchange ? s.words[kWordQueued] : s.ctrl[2];
}

/* Returns false for a call that has nothing to do; a call that cannot be served ends the
 * process. */
bool check_call(const int* nlocal_particles, const NeutralHipParticle* particles,
                const NeutralHipCrossSection* cs_scatter_table,
                const NeutralHipCrossSection* cs_absorb_table) {
  if (!(*nlocal_particles) && neutral::comm_nranks() == 1) {
    printf("Out of particles\n"); /* omp3/neutral.c:30-33 */
    fflush(stdout);
    return false;
  }
  /* (with several ranks a rank without particles still takes part: the exchanges at
   * the end of the step are collective, and on a decomposed mesh particles may arrive) */
  if (!particles || !particles->x || !particles->dead) {
    fprintf(stderr, "libneutral_hip: solve_transport_2d needs a particle store made by "
                    "this library's inject_particles (the dead[] array is required).\n");
    exit(EXIT_FAILURE);
  }
  if (cs_scatter_table->nentries < 2 || cs_absorb_table->nentries < 2) {
    fprintf(stderr, "libneutral_hip: cross-section tables need at least 2 entries.\n");
    exit(EXIT_FAILURE);
  }
  return true;
}

/* ... and what the chosen variant asks of it */
void check_variant(bool tiled, int pad, bool decomposed) {
  if (tiled && pad != 0) {
    fprintf(stderr, "libneutral_hip: the tiled variant needs pad = 0 (as main.c:33 sets).\n");
    exit(EXIT_FAILURE);
  }
  if (decomposed && !tiled) {
    fprintf(stderr, "libneutral_hip: a decomposed mesh needs the tiled variant.\n");
    exit(EXIT_FAILURE);
  }
}

/* the record of `particles` when several ranks step it: a shard, or a block's share */
State::Store* shard_of(const NeutralHipParticle* particles) {
  State::Store* shard = const_cast<State::Store*>(find_store(particles));
  const bool decomposed = shard && shard->decomposed;
  if (!decomposed && neutral::comm_nranks() == 1) {
    return nullptr;
  }
  return shard;
}

/* The kernels' arguments as the call gives them; everything the phases below fill in
 * (a.tally, a.flux_tally: begin_step_scoring) starts out null or zero. */
neutral::SolveArgs solve_args_of_call(int nx, int ny, int global_nx, int global_ny,
                                      uint64_t master_key, int pad, int x_off, int y_off, double dt,
                                      int ntotal_particles, const NeutralHipParticle* particles,
                                      const double* density, const double* edgex,
                                      const double* edgey) {
  neutral::SolveArgs a = {};
  a.tile_shift = 4;
  a.counters = g.d_counters;
  a.abort_flag = (const int*)g.d_check; /* low word of tables_check_kernel's verdict */
  a.nx = nx;
  a.ny = ny;
  a.global_nx = global_nx;
  a.global_ny = global_ny;
  a.master_key = master_key;
  a.pad = pad;
  a.x_off = x_off;
  a.y_off = y_off;
  a.dt = dt;
  a.inv_ntotal_particles = 1.0 / (double)ntotal_particles; /* omp3/neutral.c:120 */
  a.p = view_of(particles);
  a.density = density;
  a.edgex = edgex;
  a.edgey = edgey;
  return a;
}

/* the records mirror one SoA store: (re)import when they are not current */
void import_records_if_stale(Step& s, const NeutralHipParticle* particles) {
  const neutral::SolveArgs& a = s.a;
  if (g.mirror.mirrors(particles, a.nparticles)) {
    return;
  }
  g.mirror.write_back(); /* a previous owner's pending write-back */
  g.mirror.drop();
  g.tuning = neutral::launch_tuning_from_env(); /* (once per store) */
  if (s.decomposed) {
    HIP_CHECK(neutral::launch_import_by_slot(a.p, s.shard->keys, g.tiled, a.x_off, a.y_off,
                                             a.nparticles, g.stream));
  } else {
    HIP_CHECK(neutral::launch_import_records(a.p, g.tiled.rec_in, g.tiled.info_in,
                                             g.tiled.slot_of_id, g.tiled.id_in, g.tiled.tiles_x,
                                             g.tiled.tile_shift, a.x_off, a.y_off, a.nparticles,
                                             g.stream));
  }
  g.tiled.sort_end = a.nparticles; /* (no graveyard yet) */
  g.tiled.mirror_end = a.nparticles;
  g.mirror.adopt(particles, a.p, s.decomposed ? s.shard->keys : nullptr, a.nparticles);
}

/* mesh extent from the edge arrays (four doubles, once per mesh) */
void read_mesh_extent(int nx, int ny, int pad, const double* edgex, const double* edgey,
                      const double* edgedx, const double* edgedy) {
  if (g.extent_edges == (const void*)edgex && g.extent_nx == nx && g.extent_ny == ny) {
    return;
  }
  double e[4];
  HIP_CHECK(hipMemcpyAsync(&e[0], edgex + pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[1], edgex + pad + nx, sizeof(double), hipMemcpyDeviceToHost,
                           g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[2], edgey + pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[3], edgey + pad + ny, sizeof(double), hipMemcpyDeviceToHost,
                           g.stream));
  /* (and the spacings the host layer made the edges from, if the caller passes them) */
  double d[2] = {0.0, 0.0};
  if (edgedx && edgedy) {
    HIP_CHECK(hipMemcpyAsync(&d[0], edgedx + pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
    HIP_CHECK(hipMemcpyAsync(&d[1], edgedy + pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  }
  wait_for_stream();
  g.edge_dx = d[0];
  g.edge_dy = d[1];
  g.mesh_width = (e[1] > e[0]) ? e[1] - e[0] : 1.0;
  g.mesh_height = (e[3] > e[2]) ? e[3] - e[2] : 1.0;
  g.extent_edges = (const void*)edgex;
  g.extent_nx = nx;
  g.extent_ny = ny;
}

/* Periodic axes on a decomposed mesh: the global mesh's width and height as a wrap adds them,
 * W = fl(edgex[global_nx] - edgex[0]) and H likewise.  A rank that owns a block of the mesh holds
 * its own edges: the lowest first and the highest last edge over the ranks are the mesh's, the same
 * bits on every rank -- four doubles, a wait and one collective over the host links in every step
 * that has an axis set, beside the particle exchange's own (not kept by the arrays' address, which
 * a caller may reuse for another mesh).  A rank that holds the whole mesh reads nothing here: the
 * kernel that stores the step's options subtracts the edges on the device. */
void read_periodic_extent(const neutral::SolveArgs& a) {
  double e[4];
  HIP_CHECK(hipMemcpyAsync(&e[0], a.edgex + a.pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[1], a.edgex + a.pad + a.nx, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[2], a.edgey + a.pad, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipMemcpyAsync(&e[3], a.edgey + a.pad + a.ny, sizeof(double), hipMemcpyDeviceToHost, g.stream));
  wait_for_stream();
  if (a.decomposed && neutral::comm_nranks() > 1) {
    double m[4] = {-e[0], e[1], -e[2], e[3]}; /* (one collective: the maximum of -lo is -min) */
    comms_allreduce_f64(m, 4, COMMS_MAX);
    g.host_collectives++;
    e[0] = -m[0];
    e[1] = m[1];
    e[2] = -m[2];
    e[3] = m[3];
  }
  g.periodic_width = e[1] - e[0];
  g.periodic_height = e[3] - e[2];
}

/* The store the step works on: the tiled variant's records (imported when they do not mirror
 * `particles` as it stands) and what they need of the mesh; K1/K2 work on the SoA store in
 * place.  The launches' tuning is read from the environment and the runtime once per store --
 * for a store stepped for the first time, where its records are imported, or on the
 * library's first step. */
void adopt_store(Step& s, const NeutralHipParticle* particles, const double* edgedx,
                 const double* edgedy) {
  neutral::SolveArgs& a = s.a;
  if (!g.tuning_read) {
    g.tuning = neutral::launch_tuning_from_env();
    g.tuning_read = true;
  }
  if (s.tiled) {
    ensure_tiled_workspace(a.nx, a.ny, a.nparticles, s.decomposed ? s.shard->capacity : 0);
    import_records_if_stale(s, particles);
    read_mesh_extent(a.nx, a.ny, a.pad, a.edgex, a.edgey, edgedx, edgedy);
    g.tiled.slots_by_id = s.decomposed ? 0 : 1; /* (a decomposed store keeps id_out[slot] instead) */
    /* (after a possible import / pending write-back above: are the arrays current now?) */
    a.export_skip_long_dead = (s.pass_export && !s.decomposed && g.mirror.arrays_current()) ? 1 : 0;
    a.edge_dx = g.edge_dx;
    a.edge_dy = g.edge_dy;
    g.tiled.cells_per_x = (double)a.nx / g.mesh_width;
    g.tiled.cells_per_y = (double)a.ny / g.mesh_height;
  } else {
    g.mirror.write_back();
    g.mirror.arrays_rewritten(particles, /*whole_store=*/false); /* (K1/K2 step the arrays in place) */
  }
  a.steal_min = g.tuning.steal_min;
  a.steal_delay = g.tuning.steal_delay;
  a.share_weight = g.tuning.share_weight;
  a.weighted_share_min = g.tuning.weighted_share_min;
  a.compute_units = g.tuning.compute_units;
  a.max_blocks = s.tiled ? g.tuning.max_blocks : 0;
}

/* Arithmetic policy of this step's kernels (neutral_device.h).  Auto: start from what
 * the last step's check found; the check of THIS step's input runs on the device ahead
 * of the kernels and turns a fast attempt down if the input is outside the proven
 * range (the attempt then runs again, checked).  A padded mesh's halo cells hold
 * anything, so the density check cannot speak for it: checked. */
bool starts_checked(const double* density, int pad) {
  if (g.checked_density != (const void*)density) {
    g.checked_density = (const void*)density;
    g.use_checked = false;
  }
  return g.arithmetic == NEUTRAL_HIP_ARITH_CHECKED || g.use_checked || pad != 0;
}

/* Identical tables (the shipped elastic_scatter.cs / capture.cs are) need one
 * search per energy instead of two, and both searches start from a bucketed
 * index.  The view is cached and its validity checked on the device (see
 * TableView): when the check fails the kernels of this attempt have done
 * nothing, and the step runs again with a fresh view. */
void bind_table_view(Step& s, const NeutralHipCrossSection* cs_scatter_table,
                     const NeutralHipCrossSection* cs_absorb_table, bool stale_view) {
  neutral::SolveArgs& a = s.a;
  refresh_table_view(cs_scatter_table, cs_absorb_table, stale_view, !s.checked);
  const TableView& v = g.tables;
  s.same = v.same;
  a.scatter_keys = cs_scatter_table->keys;
  a.scatter_values = cs_scatter_table->values;
  a.scatter_n = cs_scatter_table->nentries;
  a.absorb_keys = cs_absorb_table->keys;
  a.absorb_values = cs_absorb_table->values;
  a.absorb_n = cs_absorb_table->nentries;
  a.same_tables = v.same;
  a.scatter_index = v.ix_s.start;
  a.scatter_index_n = v.ix_s.nbuckets;
  a.scatter_index_base = v.ix_s.base;
  a.absorb_index = v.ix_a.start;
  a.absorb_index_n = v.ix_a.nbuckets;
  a.absorb_index_base = v.ix_a.base;
  a.index_shift = v.ix_s.start ? v.ix_s.shift : v.ix_a.shift;
  g.tiled.fine_index = nullptr;
  if (s.tiled && v.fine.start) {
    g.tiled.fine_index = v.fine.start;
    g.tiled.fine_index_n = v.fine.nbuckets;
    g.tiled.fine_index_base = v.fine.base;
    g.tiled.fine_index_shift = v.fine.shift;
  }
}

/* the tally window takes 128 KB of the 160 KB of LDS: an index that does
 * not fit next to it stays in HBM-side bisection (same brackets) */
void drop_indexes_that_do_not_fit(Step& s) {
  const size_t lds_limit = 160 * 1024 - 64;
  if (neutral::tiled_lds_bytes(s.a, s.options, g.tiled) > lds_limit) {
    s.a.absorb_index = nullptr;
  }
  if (neutral::tiled_lds_bytes(s.a, s.options, g.tiled) > lds_limit) {
    s.a.scatter_index = nullptr;
  }
}

/* The write-back in two parts, when under half of the particles went to the collision stage
 * last step (csp: a tenth): the pass over the ids of everybody else runs on a stream of lowest
 * priority BESIDE the collision stage instead of after it (their records are final when the
 * stream kernel is through), and the collision stage writes the final state of the histories
 * it ends to the arrays itself (eleven scattered stores each, behind its arithmetic).
 * NEUTRAL_SPLIT_EXPORT=0: the one pass. */
neutral::SplitExport plan_split_export(Step& s) {
  neutral::SolveArgs& a = s.a;
  neutral::SplitExport split = {};
  split.on = false;
  if (s.pass_export && !s.decomposed && g.mirror.last_suspended_share() >= 0.0 &&
      g.mirror.last_suspended_share() < 0.5) {
    const char* off = getenv("NEUTRAL_SPLIT_EXPORT");
    split.on = !(off && atoi(off) == 0);
  }
  a.export_view = nullptr;
  g.tiled.mark_suspended = 0;
  if (split.on) {
    /* (the stepped store's eleven array pointers: uploaded when they change, not every step --
     * a copy out of pageable host memory is a staging kernel of 70-130 us in the kernel trace) */
    if (memcmp(&g.h_export_view, &a.p, sizeof(a.p)) != 0 || !g.export_view_uploaded) {
      g.h_export_view = a.p;
      HIP_CHECK(hipMemcpyAsync(g.d_export_view, &g.h_export_view, sizeof(a.p), hipMemcpyHostToDevice,
                               g.stream));
      g.export_view_uploaded = true;
    }
    HIP_CHECK(hipMemsetAsync(g.tiled.susp_ids, 0, sizeof(unsigned) * g.susp_id_words, g.stream));
    a.export_view = g.d_export_view;
    g.tiled.mark_suspended = 1;
    split.side = g.export_stream;
    split.done = g.ev_split_done;
    split.p = a.p;
    split.skip_long_dead = a.export_skip_long_dead;
  }
  return split;
}

/* The device's verdict on the attempt just waited for: [6] the cached view of the tables is
 * stale, [7] a fast attempt met input outside the proven range ([4] tables, [5] densities).
 * Either way the kernels of this attempt returned at entry, and it runs again -- with a fresh
 * view, with the checked instantiation.  Returns whether it was turned down. */
bool read_verdict(Step& s, bool* stale_view) {
  const unsigned long long* check = s.check;
  *stale_view = check[6] != 0;
  const bool unproven = (check[4] | check[5]) != 0;
  g.use_checked = unproven; /* (the next step starts from this) */
  if (unproven && !g.said_checked && !g.quiet) {
    g.said_checked = true;
    fprintf(stderr,
            "libneutral_hip: %s%s%s outside [2^-100, 2^100] (a true vacuum of density 0, for "
            "instance): such steps run the kernels instantiated with IEEE-checked arithmetic, "
            "which follow the reference's C on infinities and NaNs.\n",
            check[5] ? "the density of some cells lies" : "", (check[4] && check[5]) ? " and " : "",
            check[4] ? "some cross-section table entries lie" : "");
  }
  if (check[7] != 0) {
    s.checked = true;
  }
  /* (several ranks take every decision that leads to another exchange together:
   * the collectives must pair up) */
  return s.exchange ? s.words[kWordTurnedDown] != 0 : check[0] != 0;
}

/* Enqueues the step and waits for it, once in a steady state; again when the device turned
 * the attempt down. */
void run_attempts(Step& s, const NeutralHipCrossSection* cs_scatter_table,
                  const NeutralHipCrossSection* cs_absorb_table, const double* density,
                  double* energy_deposition_tally) {
  neutral::SolveArgs& a = s.a;
  bool stale_view = false;
  for (int attempt = 0;; ++attempt) {
    s.attempts++;
    /* is every density inside the proven range?  Asked every step, like the tables (a
     * pass over nx * ny doubles: microseconds), read with the step's counters */
    HIP_CHECK(hipMemsetAsync(g.d_check + 5, 0, sizeof(unsigned long long), g.stream));
    if (a.pad == 0) {
      HIP_CHECK(neutral::launch_unphysical_values(density, (long long)a.nx * a.ny, g.d_check + 5,
                                                  g.stream));
    }
    a.checked = s.checked ? 1 : 0;
    bind_table_view(s, cs_scatter_table, cs_absorb_table, stale_view);
    s.options = begin_step_scoring(a, energy_deposition_tally, s.tiled, s.exchange);
    HIP_CHECK(neutral::set_step_options(s.options, g.stream));
    if (s.tiled) {
      drop_indexes_that_do_not_fit(s);
    }
    if (s.tiled && neutral::tiled_uses_carried(a, g.tiled) && !g.mirror.carried_current()) {
      /* the stream kernel starts histories from the cross section carried with each record:
       * looked up here for a store just imported, or after the table view was rebuilt (an
       * attempt that is turned down for a stale view comes back through here) */
      HIP_CHECK(neutral::launch_refresh_micro(a, g.tiled, g.stream));
      g.mirror.carried_refreshed();
    }
    HIP_CHECK(hipMemsetAsync(g.d_counters, 0, 2 * sizeof(neutral::StepCounters), g.stream));
    if (s.tiled) {
      /* (the pipeline's control words are set by its own kernels -- unless there is
       * nothing to launch them for: a rank that starts the step without particles) */
      HIP_CHECK(hipMemsetAsync(g.tiled.ctrl, 0, sizeof(unsigned) * 16, g.stream));
    }
    const neutral::SplitExport split = plan_split_export(s);
    s.stage = StageMs(); /* (an attempt that was turned down did nothing worth timing ... */
    s.queue_total = 0;   /*  ... or counting) */
    run_batch(s, first_batch(split.on ? &split : nullptr));
    s.local_nprocessed = s.hc[0].nprocessed + s.hc[1].nprocessed;
    if (!read_verdict(s, &stale_view)) {
      return;
    }
    if (attempt >= 3) {
      fprintf(stderr, "libneutral_hip: the cross-section tables keep changing under "
                      "solve_transport_2d.\n");
      exit(EXIT_FAILURE);
    }
  }
}

/* Finishes what is enqueued: migrants left over mean the step outran the plan (it
 * needs more stream passes than the last one did).  More passes, as many again as
 * have run; the histories they suspend get a collision stage of their own (the
 * first one's are marked done), and with several ranks their tallies an exchange
 * of their own. */
void finish_passes(Step& s) {
  while (s.exchange ? (s.words[kWordMigrants] != 0) : (s.ctrl[4] != 0)) {
    run_batch(s, later_batch(s.passes < 2 ? 2 : s.passes, s.passes));
  }
}

/* Decomposed mesh: histories that crossed into another rank's block wait as
 * emigrants.  Rounds of: count and pack them by destination, exchange, append
 * the arrivals, go on with the step for them -- until no rank has any. */
void run_emigrant_rounds(Step& s) {
  for (;;) {
    uint64_t waiting = s.ctrl[7];
    comms_allreduce_u64(&waiting, 1, COMMS_SUM);
    g.host_collectives++;
    if (waiting == 0) {
      return;
    }
    const int arrived = exchange_particles(s.a, g.tiled);
    s.a.nparticles += arrived;
    /* (pass 0 would start histories over) */
    run_batch(s, later_batch(2, s.passes < 1 ? 1 : s.passes));
    finish_passes(s);
  }
}

/* ... and then the particles that are here now, without the holes the emigrants left; they
 * land in the other record buffer, which is where the next step looks */
void compact_decomposed_store(Step& s, int* nlocal_particles) {
  const neutral::SolveArgs& a = s.a;
  unsigned kept = 0;
  HIP_CHECK(neutral::launch_compact_records(g.tiled, a.nparticles, g.d_exchange + 192,
                                            g.stream));
  HIP_CHECK(hipMemcpyAsync(&kept, g.d_exchange + 192, sizeof(unsigned), hipMemcpyDeviceToHost,
                           g.stream));
  wait_for_stream();
  s.shard->count = (int)kept;
  *nlocal_particles = (int)kept;
  g.mirror.compacted((int)kept);
  if (s.pass_export) {
    HIP_CHECK(hipEventRecord(g.ev_stop, g.stream));
    HIP_CHECK(neutral::launch_export_by_slot(g.tiled.rec_in, a.p, s.shard->keys, (int)kept,
                                             g.stream));
    HIP_CHECK(hipEventRecord(g.ev_exported, g.stream));
    wait_for_stream();
    float ms_slot = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms_slot, g.ev_stop, g.ev_exported));
    s.stage.exported += (double)ms_slot;
  }
}

/* What the tiled variant keeps for the next step of this store; this step's records become
 * its input (a decomposed store's compaction has put them there already). */
void roll_records(const Step& s) {
  neutral::TiledArgs& t = g.tiled;
  if (!s.decomposed) {
    std::swap(t.rec_in, t.rec_out);
    std::swap(t.info_in, t.info_out);
    std::swap(t.id_in, t.id_out);
    std::swap(t.carried_in, t.carried_out);
    /* the graveyard grows by what the sort carried over a step ago; what it carried over
     * now joins next step (ctrl[8]: the first slot of the dead this step's sort found) */
    t.mirror_end = t.sort_end;
    t.sort_end = ((int)s.ctrl[8] <= t.sort_end) ? (int)s.ctrl[8] : t.sort_end;
  }
  const double share = (double)s.queue_total / ((double)(s.a.nparticles > 0 ? s.a.nparticles : 1) *
                                                (double)neutral::comm_nranks());
  g.mirror.rolled((int)s.ctrl[5], g.lazy_export != 0, !s.decomposed, t.carried != 0, share, t.sort_end);
}

typedef unsigned long long neutral::StepCounters::*CounterField;
/* The step words that carry event counters (StepWord): one word per kernel record for the
 * four event counts, from kWordCounters on ... */
const CounterField kWordsPerKernel[4] = {&neutral::StepCounters::nprocessed, &neutral::StepCounters::nfacets,
                                         &neutral::StepCounters::ncollisions, &neutral::StepCounters::ncensus};
/* ... and one word for both records' sum, which the second record is given */
const struct { int word; CounterField field; } kWordsOfBoth[] = {
    {kWordRequeued, &neutral::StepCounters::nrequeued},
    {kWordCollidePasses, &neutral::StepCounters::ncollide_passes},
    {kWordSteals, &neutral::StepCounters::nsteals},
    {kWordStealsRefused, &neutral::StepCounters::steal_refused},
    {kWordWeightedWaves, &neutral::StepCounters::nweighted},
    {kWordRouletteKilled, &neutral::StepCounters::roulette_killed},
    {kWordRouletteSurvived, &neutral::StepCounters::roulette_survived},
};

/* The step's counters (and the collision queue's length) of all ranks, in s.hc and
 * s.queue_total. */
void reduce_counters_over_ranks(Step& s) {
  neutral::StepCounters* hc = s.hc;
  if (s.exchange) {
    /* they travelled with the tally (StepWord) */
    for (int k = 0; k < 2; ++k) {
      for (int f = 0; f < 4; ++f) {
        hc[k].*kWordsPerKernel[f] = s.words[kWordCounters + 4 * k + f];
      }
    }
    for (const auto& w : kWordsOfBoth) {
      hc[0].*w.field = 0;
      hc[1].*w.field = s.words[w.word];
    }
    hc[0].aborted = 0;
    hc[1].aborted = (unsigned)s.words[kWordAborted];
    hc[0].roulette_weight_lost = 0.0;
    hc[1].roulette_weight_lost = g.h_results->roulette_weights[0]; /* (the last publication's) */
    hc[0].roulette_weight_gained = 0.0;
    hc[1].roulette_weight_gained = g.h_results->roulette_weights[1];
    for (int side = 0; side < 4; ++side) { /* (the escapes rode the same all-reduce) */
      hc[0].escaped[side] = 0;
      hc[1].escaped[side] = (unsigned long long)g.h_results->escape[side];
      hc[0].escape_weight[side] = 0.0;
      hc[1].escape_weight[side] = g.h_results->escape[4 + side];
      hc[0].wrapped[side] = 0; /* (... and so did the wraps) */
      hc[1].wrapped[side] = (unsigned long long)g.h_results->wrap[side];
      hc[0].wrap_weight[side] = 0.0;
      hc[1].wrap_weight[side] = g.h_results->wrap[4 + side];
    }
  } else if (neutral::comm_nranks() > 1) {
    /* decomposed mesh: a handful of words over the host links, like its other exchanges */
    static_assert(sizeof(Step::hc) % 8 == 0, "StepCounters is summed word by word");
    const unsigned aborted[2] = {hc[0].aborted, hc[1].aborted};
    /* (the weights roulette moved are doubles: summed as doubles, when it is on) */
    double roulette_weights[2] = {hc[0].roulette_weight_lost + hc[1].roulette_weight_lost,
                                  hc[0].roulette_weight_gained + hc[1].roulette_weight_gained};
    /* (likewise, when a side is vacuum or an axis periodic: the escapes' weights, then the wraps';
     * the counts are words like the others) */
    double escape_weights[8];
    for (int side = 0; side < 4; ++side) {
      escape_weights[side] = hc[0].escape_weight[side] + hc[1].escape_weight[side];
      escape_weights[4 + side] = hc[0].wrap_weight[side] + hc[1].wrap_weight[side];
    }
    comms_allreduce_u64((uint64_t*)hc, sizeof(Step::hc) / 8, COMMS_SUM);
    hc[0].aborted = aborted[0]; /* (two 32-bit fields share a word: keep the local ones) */
    hc[1].aborted = aborted[1];
    uint64_t q = s.queue_total;
    comms_allreduce_u64(&q, 1, COMMS_SUM);
    s.queue_total = q;
    g.host_collectives += 2;
    if (g.roulette_plays()) {
      comms_allreduce_f64(roulette_weights, 2, COMMS_SUM);
      g.host_collectives++;
    } else {
      roulette_weights[0] = roulette_weights[1] = 0.0;
    }
    hc[0].roulette_weight_lost = roulette_weights[0];
    hc[1].roulette_weight_lost = 0.0;
    hc[0].roulette_weight_gained = roulette_weights[1];
    hc[1].roulette_weight_gained = 0.0;
    if (g.vacuum_sides != 0 || g.periodic_axes != 0) {
      comms_allreduce_f64(escape_weights, g.periodic_axes != 0 ? 8 : 4, COMMS_SUM);
      g.host_collectives++;
    }
    for (int side = 0; side < 4; ++side) {
      hc[0].escape_weight[side] = g.vacuum_sides != 0 ? escape_weights[side] : 0.0;
      hc[1].escape_weight[side] = 0.0;
      hc[0].wrap_weight[side] = g.periodic_axes != 0 ? escape_weights[4 + side] : 0.0;
      hc[1].wrap_weight[side] = 0.0;
    }
  }
}

/* the step as the caller sees it: its event totals, NeutralHipStepStats, the two prints */
void report_step(const Step& s, uint64_t* facet_events, uint64_t* collision_events) {
  const neutral::StepCounters* hc = s.hc;
  const bool tiled = s.tiled;
  neutral::StepCounters h = hc[0];
  h.nprocessed += hc[1].nprocessed;
  h.nfacets += hc[1].nfacets;
  h.ncollisions += hc[1].ncollisions;
  h.ncensus += hc[1].ncensus;

  *facet_events += h.nfacets; /* omp3/neutral.c:202-203 */
  *collision_events += h.ncollisions;

  g.last.nprocessed = h.nprocessed;
  g.last.facets = h.nfacets;
  g.last.collisions = h.ncollisions;
  g.last.census = h.ncensus;
  g.last.kernel_ms = s.stage.kernel;
  g.last.same_tables = s.same;
  g.last.variant = g.variant;
  /* sort_ms: the first sort and the queue builds (later sorts sit inside stream_ms) */
  g.last.sort_ms = s.stage.sort;
  g.last.stream_ms = s.stage.stream;
  g.last.collide_ms = s.stage.collide;
  g.last.stream_facets = tiled ? hc[0].nfacets : 0;
  g.last.stream_census = tiled ? hc[0].ncensus : 0;
  g.last.suspended = s.queue_total;
  g.last.aborted = (uint64_t)hc[0].aborted + (uint64_t)hc[1].aborted;
  if (g.last.aborted) {
    fprintf(stderr, "libneutral_hip: warning: %llu histories exceeded the event watchdog or were "
                    "dropped by a consistency check of the stream kernel's tile queues, and were "
                    "stopped: the step's results are incomplete.\n", (unsigned long long)g.last.aborted);
  }
  g.last.stream_passes = tiled ? (int)s.ctrl[5] : 0;
  g.last.requeued = tiled ? hc[1].nrequeued : 0;
  g.last.collide_passes = hc[0].ncollide_passes + hc[1].ncollide_passes;
  g.last.steals = hc[0].nsteals + hc[1].nsteals;
  g.last.steals_refused = hc[0].steal_refused + hc[1].steal_refused;
  g.last.weighted_waves = hc[0].nweighted + hc[1].nweighted;
  /* (this rank's own launches: the clocks are not summed over ranks) */
  g.last.stream_clock_ghz = hc[0].clock_100mhz_ticks
                                ? (double)hc[0].clock_shader_ticks / ((double)hc[0].clock_100mhz_ticks * 10.0)
                                : 0.0;
  g.last.collide_clock_ghz = hc[1].clock_100mhz_ticks
                                 ? (double)hc[1].clock_shader_ticks / ((double)hc[1].clock_100mhz_ticks * 10.0)
                                 : 0.0;
  g.last.stream_hops = tiled ? s.ctrl[10] : 0;
  g.last.stream_overflows = tiled ? s.ctrl[11] : 0;
  g.last.stream_batches = tiled ? s.ctrl[12] : 0;
  g.last.stream_idle_polls = tiled ? s.ctrl[13] : 0;
  g.last.local_nprocessed = s.local_nprocessed;
  g.last.exchange_ms = s.stage.exchange;
  g.last.exchange_rounds = g.exchange_rounds;
  g.last.emigrants = g.emigrants;
  g.last.host_syncs = g.host_syncs;
  g.last.stream_passes_enqueued = tiled ? s.passes : 0;
  g.last.tile_cells = tiled ? (1 << g.tiled.tile_shift) : 0;
  g.last.export_ms = s.stage.exported;
  g.last.checked_arithmetic = s.checked ? 1 : 0;
  g.last.attempts = s.attempts;
  g.last.host_collectives = g.host_collectives;
  g.last.exchange_ranks = s.exchange ? (int)s.words[kWordRanks] : 1;
  g.last.roulette_killed = hc[0].roulette_killed + hc[1].roulette_killed;
  g.last.roulette_survived = hc[0].roulette_survived + hc[1].roulette_survived;
  g.last.roulette_weight_lost = hc[0].roulette_weight_lost + hc[1].roulette_weight_lost;
  g.last.roulette_weight_gained = hc[0].roulette_weight_gained + hc[1].roulette_weight_gained;
  for (int side = 0; side < 4; ++side) { /* (neutral_hip_last_escape: not NeutralHipStepStats, whose size is pinned) */
    g.last_escape.escaped[side] = hc[0].escaped[side] + hc[1].escaped[side];
    g.last_escape.weight[side] = hc[0].escape_weight[side] + hc[1].escape_weight[side];
    g.last_wraps.wrapped[side] = hc[0].wrapped[side] + hc[1].wrapped[side]; /* (neutral_hip_last_wraps) */
    g.last_wraps.weight[side] = hc[0].wrap_weight[side] + hc[1].wrap_weight[side];
  }
  /* (the escape bank: this rank's own cursor, as the step's last publication carried it) */
  const uint64_t bank_before = g.bank_claimed, recorded_before = g.bank_recorded();
  if (g.bank_recording) {
    g.bank_claimed = g.h_results->bank_cursor;
  }
  g.bank_step_claimed = g.bank_claimed - bank_before;
  g.bank_step_recorded = g.bank_recorded() - recorded_before;

  if (!g.quiet) {
    printf("Particles  %llu\n", (unsigned long long)h.nprocessed); /* omp3/neutral.c:205 */
    fflush(stdout);
  }
}

}  // namespace

extern "C" {

/* ---- 1. reference kernel interface ------------------------------------------ */

void solve_transport_2d(const int nx, const int ny, const int global_nx, const int global_ny,
                        const uint64_t master_key, const int pad, const int x_off,
                        const int y_off, const double dt, const int ntotal_particles,
                        int* nlocal_particles, const int* neighbours,
                        NeutralHipParticle* particles, const double* density,
                        const double* edgex, const double* edgey, const double* edgedx,
                        const double* edgedy, NeutralHipCrossSection* cs_scatter_table,
                        NeutralHipCrossSection* cs_absorb_table,
                        double* energy_deposition_tally, uint64_t* reduce_array0,
                        uint64_t* reduce_array1, uint64_t* reduce_array2,
                        uint64_t* facet_events, uint64_t* collision_events) {
  (void)neighbours;
  (void)reduce_array0;
  (void)reduce_array1;
  (void)reduce_array2;

  if (!check_call(nlocal_particles, particles, cs_scatter_table, cs_absorb_table)) {
    return;
  }
  read_variant_env();
  ensure_scratch();
  g.host_syncs = 0;
  g.host_collectives = 0;
  g.exchange_rounds = 0;
  g.emigrants = 0;

  Step s;
  s.tiled = (g.variant == NEUTRAL_HIP_VARIANT_TILED);
  s.shard = shard_of(particles);
  s.decomposed = s.shard && s.shard->decomposed;
  check_variant(s.tiled, pad, s.decomposed);
  s.exchange = neutral::comm_nranks() > 1 && !s.decomposed;
  /* Default (eager) mode: the SoA arrays are current when the call returns.  One
   * export pass at the end of the step does that (5.9 ms at 1e8 particles); letting
   * every kernel that ends a history store it to the arrays itself -- eleven
   * scattered 8-byte stores per history -- cost 18 ms (profiles/r02: fused export). */
  s.pass_export = s.tiled && !g.lazy_export;
  s.a = solve_args_of_call(nx, ny, global_nx, global_ny, master_key, pad, x_off, y_off, dt,
                           ntotal_particles, particles, density, edgex, edgey);
  s.a.nparticles = s.shard ? s.shard->count : *nlocal_particles;
  s.a.pid_base = s.decomposed ? 0 : (s.shard ? s.shard->first : g.pid_base);
  s.a.decomposed = s.decomposed ? 1 : 0;
  if (g.vacuum_sides != 0 && s.tiled && (s.decomposed ? s.shard->capacity : s.a.nparticles) >= (1 << 30)) {
    /* (the stream kernel carries "escaped" in bit 30 of a history's id: neutral_history.h) */
    fprintf(stderr, "libneutral_hip: vacuum sides need a store of fewer than 2^30 particles in the tiled variant.\n");
    exit(EXIT_FAILURE);
  }

  if (g.periodic_axes != 0 && s.decomposed) {
    read_periodic_extent(s.a); /* (one rank, particle shards: on the device, neutral_step_options.h) */
  }
  adopt_store(s, particles, edgedx, edgedy);
  s.checked = starts_checked(density, pad);
  run_attempts(s, cs_scatter_table, cs_absorb_table, density, energy_deposition_tally);
  if (s.tiled) {
    finish_passes(s);
    if (s.decomposed) {
      run_emigrant_rounds(s);
      compact_decomposed_store(s, nlocal_particles);
    }
    roll_records(s);
  }
  reduce_counters_over_ranks(s);
  report_step(s, facet_events, collision_events);
}

size_t inject_particles(const int nparticles, const int global_nx, const int local_nx,
                        const int local_ny, const int pad,
                        const double local_particle_left_off,
                        const double local_particle_bottom_off,
                        const double local_particle_width,
                        const double local_particle_height, const int x_off, const int y_off,
                        const double dt, const double* edgex, const double* edgey,
                        const double initial_energy, NeutralHipParticle** particles) {
  (void)global_nx;
  NeutralHipParticle* p = (NeutralHipParticle*)malloc(sizeof(NeutralHipParticle));
  if (!p) {
    fprintf(stderr, "Could not allocate particle array.\n"); /* omp3/neutral.c:571-573 */
    exit(EXIT_FAILURE);
  }
  /* several ranks: this rank's contiguous share of the ids 0..nparticles-1 (the
   * OpenMP static split of omp3/neutral.c:64-74 over ranks); ids stay global, so
   * every history is the one a single rank would run */
  int local = nparticles > 0 ? nparticles : 0;
  const bool decomposed = g.domain_on && (local_nx < global_nx || g.domain.px * g.domain.py > 1);
  const bool sharded = !decomposed && neutral::comm_nranks() > 1 && g.auto_shard;
  if (sharded) {
    long long first = 0, count = 0;
    comms_shard_range(local, neutral::comm_rank(), neutral::comm_nranks(), &first, &count);
    g.pid_base = (uint64_t)first;
    local = (int)count;
  }
  const size_t n = (size_t)local;
  size_t allocation = 0;
  double** f64[] = {&p->x,      &p->y,      &p->omega_x,      &p->omega_y,
                    &p->energy, &p->weight, &p->dt_to_census, &p->mfp_to_collision};
  for (double** f : f64) {
    *f = (double*)device_zalloc(sizeof(double) * n);
    allocation += sizeof(double) * n;
  }
  int** i32[] = {&p->cellx, &p->celly, &p->dead};
  for (int** f : i32) {
    *f = (int*)device_zalloc(sizeof(int) * n);
    allocation += sizeof(int) * n;
  }
  *particles = p;
  if (sharded) {
    remember_store(p, local, g.pid_base);
  }
  if (decomposed) {
    /* Decomposed mesh: the store has room for every particle of the problem (any of
     * them may pass through this rank's block) and starts with the ones the source
     * puts there.  `nparticles` and the particle box are the GLOBAL ones: every rank
     * looks at all candidates, so that each particle is what one rank alone would
     * have made of it. */
    State::Store* st = remember_store(p, 0, 0);
    st->decomposed = true;
    st->capacity = local;
    HIP_CHECK(hipMalloc((void**)&st->keys, sizeof(unsigned) * (n ? n : 1)));
    allocation += sizeof(unsigned) * n;
    run_inject_filtered(st, nparticles, local_nx, local_ny, pad, local_particle_left_off,
                        local_particle_bottom_off, local_particle_width, local_particle_height,
                        x_off, y_off, dt, edgex, edgey, initial_energy, p);
    return allocation;
  }

  run_inject(local, local_nx, local_ny, pad, local_particle_left_off,
             local_particle_bottom_off, local_particle_width, local_particle_height, x_off,
             y_off, dt, edgex, edgey, initial_energy, p);
  return allocation;
}

void validate(const int nx, const int ny, const char* params_filename, const int rank,
              double* energy_tally) {
  const size_t ncells = (size_t)nx * (size_t)ny;
  double* h_tally = (double*)malloc(sizeof(double) * (ncells ? ncells : 1));
  if (!h_tally) {
    fprintf(stderr, "Could not allocate the host tally.\n");
    exit(EXIT_FAILURE);
  }
  HIP_CHECK(hipMemcpyAsync(h_tally, energy_tally, sizeof(double) * ncells,
                           hipMemcpyDeviceToHost, g.stream));
  HIP_CHECK(hipStreamSynchronize(g.stream));

  /* serial sum in index order, omp3/neutral.c:524-527 */
  double global_energy_tally = 0.0;
  for (size_t ii = 0; ii < ncells; ++ii) {
    global_energy_tally += h_tally[ii];
  }
  free(h_tally);
  if (g.domain_on && neutral::comm_nranks() > 1) {
    /* decomposed mesh: every rank holds the tally of its own cells (omp3/neutral.c:530) */
    comms_allreduce_f64(&global_energy_tally, 1, COMMS_SUM);
  }

  if (rank != 0) {
    return;
  }
  printf("\nFinal global_energy_tally %.15e\n", global_energy_tally);

  int nresults = 0;
  char* keys = (char*)malloc(sizeof(char) * NEUTRAL_MAX_KEYS * (NEUTRAL_MAX_STR_LEN + 1));
  double* values = (double*)malloc(sizeof(double) * NEUTRAL_MAX_KEYS);
  if (!keys || !values ||
      !get_key_value_parameter(params_filename, g.tests_file, keys, values, &nresults) ||
      nresults < 1) {
    printf("Warning. Test entry was not found, could NOT validate.\n");
    fflush(stdout);
    free(keys);
    free(values);
    return;
  }
  printf("Expected %.12e, result was %.12e.\n", values[0], global_energy_tally);
  if (within_tolerance(values[0], global_energy_tally, NEUTRAL_VALIDATE_TOLERANCE)) {
    printf("PASSED validation.\n");
  } else {
    printf("FAILED validation.\n");
  }
  fflush(stdout);
  free(keys);
  free(values);
}

/* ---- 2. allocation hooks, HBM flavour ---------------------------------------- */

}  // extern "C"
