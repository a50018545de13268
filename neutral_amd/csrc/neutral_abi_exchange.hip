/*
 * neutral_abi_exchange.hip -- what leaves the device at the end of a batch of launches: the
 * step's results published into pinned host memory, the tally exchange between the ranks of a
 * sharded run (one all-reduce per step, the event counters riding on a second one), and the
 * particle exchange between the blocks of a decomposed mesh.  Host code and three small kernels.
 */
#include "neutral_abi_state.h"

namespace neutral_abi {

/* the step's results, into the pinned block the host reads after its wait (one workgroup) */
__global__ void publish_results_kernel(const neutral::StepCounters* counters,
                                       const unsigned long long* check, const unsigned* ctrl,
                                       const unsigned long long* words,
                                       const double* roulette_weights,
                                       const unsigned long long* bank_cursor, StepResults* out) {
  const unsigned t = threadIdx.x;
  const unsigned* c32 = (const unsigned*)counters;
  unsigned* o32 = (unsigned*)out->counters;
  for (unsigned i = t; i < 2 * sizeof(neutral::StepCounters) / 4; i += blockDim.x) {
    o32[i] = c32[i];
  }
  if (t < 8) out->check[t] = check[t];
  if (t < 16) out->ctrl[t] = ctrl ? ctrl[t] : 0u;
  if (t < (unsigned)kStepWords) out->words[t] = words ? words[t] : 0ull;
  if (t < 2) out->roulette_weights[t] = roulette_weights ? roulette_weights[t] : 0.0;
  /* (the step's scalars: the escapes follow the two weights) */
  if (t < 8) out->escape[t] = roulette_weights ? roulette_weights[kScalarEscaped + t] : 0.0;
  if (t < 8) out->wrap[t] = roulette_weights ? roulette_weights[kScalarWrapped + t] : 0.0; /* (... and the wraps) */
  /* (the escape bank's cursor, where this step records: read with the rest, no copy of its own) */
  if (t == 0) out->bank_cursor = bank_cursor ? *bank_cursor : 0ull;
}

__global__ void pack_step_words_kernel(const neutral::StepCounters* c, const unsigned long long* check,
                                       const unsigned* ctrl, unsigned long long* w,
                                       double* scalars) {
  if (threadIdx.x != 0) {
    return;
  }
  for (int k = 0; k < 2; ++k) {
    w[kWordCounters + 4 * k + 0] = c[k].nprocessed;
    w[kWordCounters + 4 * k + 1] = c[k].nfacets;
    w[kWordCounters + 4 * k + 2] = c[k].ncollisions;
    w[kWordCounters + 4 * k + 3] = c[k].ncensus;
  }
  w[kWordRequeued] = c[0].nrequeued + c[1].nrequeued;
  w[kWordCollidePasses] = c[0].ncollide_passes + c[1].ncollide_passes;
  w[kWordTurnedDown] = check[0] ? 1ull : 0ull;
  w[kWordMigrants] = ctrl ? ctrl[4] : 0u;
  w[kWordQueued] = ctrl ? ctrl[2] : 0u;
  w[kWordAborted] = (unsigned long long)c[0].aborted + c[1].aborted;
  w[kWordRanks] = 1ull;
  w[kWordSteals] = c[0].nsteals + c[1].nsteals;
  w[kWordStealsRefused] = c[0].steal_refused + c[1].steal_refused;
  w[kWordWeightedWaves] = c[0].nweighted + c[1].nweighted;
  w[kWordRouletteKilled] = c[0].roulette_killed + c[1].roulette_killed;
  w[kWordRouletteSurvived] = c[0].roulette_survived + c[1].roulette_survived;
  scalars[kScalarRouletteLost] = c[0].roulette_weight_lost + c[1].roulette_weight_lost;
  scalars[kScalarRouletteGained] = c[0].roulette_weight_gained + c[1].roulette_weight_gained;
  for (int side = 0; side < 4; ++side) {
    scalars[kScalarEscaped + side] = (double)(c[0].escaped[side] + c[1].escaped[side]);
    scalars[kScalarEscapeWeight + side] = c[0].escape_weight[side] + c[1].escape_weight[side];
    scalars[kScalarWrapped + side] = (double)(c[0].wrapped[side] + c[1].wrapped[side]);
    scalars[kScalarWrapWeight + side] = c[0].wrap_weight[side] + c[1].wrap_weight[side];
  }
}

__global__ void add_step_tally_kernel(double* __restrict__ tally, const double* __restrict__ step,
                                      size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    tally[i] += step[i];
  }
}

/* n values of a step buffer into the caller's array */
static void add_to_caller(double* caller, const double* step, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(add_step_tally_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, caller, step, n);
  HIP_CHECK(hipGetLastError());
}

/* What the step scored into buffers, into the caller's arrays; the buffers are cleared again,
 * so a step that needs more stream passes than were enqueued simply adds what those score.
 * `reduce`: several ranks share the mesh, and each buffer is summed over them first -- ONE
 * all-reduce (sum, f64) per tally on the stream, in the table's order on every rank; the sum
 * joins the caller's mesh, which then holds the same global tally on every rank.  (The spectrum
 * was summed with the step's scalars: exchange_step.) */
static void step_buffers_to_caller(const neutral::SolveArgs& a, bool reduce, hipStream_t s) {
  if (g.spectrum_out) {
    const size_t n = 2 * (size_t)g.spectrum_ngroups;
    add_to_caller(g.spectrum_out, g.d_step_scalars + kScalarSpectrum, n, s);
    HIP_CHECK(hipMemsetAsync(g.d_step_scalars + kScalarSpectrum, 0, sizeof(double) * n, s));
  }
  if (g.leakage_scored) {
    /* (the leakage tally: its bins are no mesh and up to 2 * 4 * 65 * 64 values, so it is neither
     * a MeshTally nor a guest of the step's scalars -- one all-reduce of its own where the ranks
     * share the mesh) */
    const size_t n = 2 * g.leakage_bins();
    if (reduce) {
      neutral::comm_allreduce_sum(g.leakage_scored, n, true, s);
    }
    add_to_caller(g.leakage_out, g.leakage_scored, n, s);
    HIP_CHECK(hipMemsetAsync(g.leakage_scored, 0, sizeof(double) * n, s));
  }
  const size_t ncells = (size_t)a.nx * (size_t)a.ny;
  for (const MeshTally& t : g.tallies) {
    if (!t.scored) {
      continue;
    }
    if (!t.caller[0]) {
      /* (the outflow's buffer under vacuum sides alone: scored for the rule's sake, read by nobody) */
      HIP_CHECK(hipMemsetAsync(t.scored, 0, sizeof(double) * (size_t)t.meshes * ncells, s));
      continue;
    }
    if (reduce) {
      neutral::comm_allreduce_sum(t.scored, (size_t)t.meshes * ncells, true, s);
    }
    for (int m = 0; m < t.meshes; ++m) {
      add_to_caller(t.caller[m], t.scored + (size_t)m * ncells, ncells, s);
    }
    HIP_CHECK(hipMemsetAsync(t.scored, 0, sizeof(double) * (size_t)t.meshes * ncells, s));
  }
}

void tallies_to_caller(const neutral::SolveArgs& a) { step_buffers_to_caller(a, false, g.stream); }

void exchange_step(const neutral::SolveArgs& a, bool tiled) {
  /* on a stream of its own, after the step's kernels (g.ev_stop) and BESIDE the write-back
   * of the records that the caller enqueues next on its own stream; finish_exchange() joins */
  hipStream_t xs = g.comm_stream;
  HIP_CHECK(hipStreamWaitEvent(xs, g.ev_stop, 0));
  HIP_CHECK(hipEventRecord(g.ev_exchange_begins, xs));
  hipLaunchKernelGGL(pack_step_words_kernel, dim3(1), dim3(64), 0, xs, g.d_counters, g.d_check,
                     tiled ? (const unsigned*)g.tiled.ctrl : (const unsigned*)nullptr, g.d_words,
                     g.d_step_scalars);
  HIP_CHECK(hipGetLastError());
  neutral::comm_allreduce_sum(g.d_words, (size_t)kStepWords, false, xs);
  if (g.roulette_plays() || g.spectrum_out || g.vacuum_sides != 0 || g.periodic_axes != 0) {
    /* (the weights roulette moved: f64, not step words; the escapes, the wraps and the spectrum
     * behind them) */
    neutral::comm_allreduce_sum(g.d_step_scalars,
                                kScalarSpectrum + (g.spectrum_out ? 2 * (size_t)g.spectrum_ngroups : 0), true, xs);
  }
  step_buffers_to_caller(a, true, xs);
  HIP_CHECK(hipEventRecord(g.ev_exchanged, xs));
}

/* the caller's stream goes on only when the exchange is done (the step buffers are reused) */
void finish_exchange() { HIP_CHECK(hipStreamWaitEvent(g.stream, g.ev_exchanged, 0)); }

/* enqueues the publication of the batch's results; fetch_results() after the wait */
void publish_results(bool tiled, bool with_words) {
  hipLaunchKernelGGL(publish_results_kernel, dim3(1), dim3(64), 0, g.stream, g.d_counters, g.d_check,
                     tiled ? (const unsigned*)g.tiled.ctrl : (const unsigned*)nullptr,
                     with_words ? (const unsigned long long*)g.d_words
                                : (const unsigned long long*)nullptr,
                     with_words ? (const double*)g.d_step_scalars : (const double*)nullptr,
                     g.bank_recording ? (const unsigned long long*)g.bank_cursor.d : (const unsigned long long*)nullptr,
                     g.d_results);
  HIP_CHECK(hipGetLastError());
}

void fetch_results(neutral::StepCounters* hc, unsigned long long* check, unsigned* ctrl,
                   unsigned long long* words) {
  const StepResults& r = *g.h_results;
  memcpy(hc, r.counters, sizeof(r.counters));
  if (check) memcpy(check, r.check, sizeof(r.check));
  if (ctrl) memcpy(ctrl, r.ctrl, sizeof(r.ctrl));
  if (words) memcpy(words, r.words, sizeof(r.words));
}

/* Decomposed mesh, one round: this rank's emigrants (records of t.rec_out marked
 * kRecEmigrate) go to the ranks that own the cells they crossed into; what arrives
 * is appended behind the a.nparticles records already here, as migrants.  Returns the
 * number of arrivals.  Collective over the ranks. */
int exchange_particles(const neutral::SolveArgs& a, neutral::TiledArgs& t) {
  const int n = neutral::comm_nranks();
  const int me = neutral::comm_rank();
  if (n > 64) {
    fprintf(stderr, "libneutral_hip: the decomposed-mesh exchange handles up to 64 ranks.\n");
    exit(EXIT_FAILURE);
  }
  unsigned* d_counts = g.d_exchange;
  unsigned* d_offsets = g.d_exchange + 64;
  unsigned* d_cursor = g.d_exchange + 128;
  HIP_CHECK(hipMemsetAsync(g.d_exchange, 0, sizeof(unsigned) * 192, g.stream));
  HIP_CHECK(neutral::launch_emigrant_count(t, a.nparticles, g.domain, d_counts, g.stream));
  unsigned counts[64];
  HIP_CHECK(hipMemcpyAsync(counts, d_counts, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost,
                           g.stream));
  wait_for_stream();
  uint64_t matrix[64 * 64];
  memset(matrix, 0, sizeof(uint64_t) * (size_t)n * n);
  unsigned offsets[64];
  size_t out = 0;
  for (int d = 0; d < n; ++d) {
    offsets[d] = (unsigned)out;
    out += counts[d];
    matrix[(size_t)me * n + d] = (uint64_t)counts[d] * sizeof(neutral::ParticleRec);
  }
  if (counts[me] != 0) {
    fprintf(stderr, "libneutral_hip: rank %d: %u emigrants are bound for their own rank (the "
                    "decomposition given to neutral_hip_set_decomposition does not match the "
                    "mesh blocks passed to solve_transport_2d).\n", me, counts[me]);
    exit(EXIT_FAILURE);
  }
  comms_allreduce_u64(matrix, (size_t)n * n, COMMS_SUM);
  g.host_collectives++;
  size_t in = 0;
  for (int s2 = 0; s2 < n; ++s2) {
    in += (size_t)(matrix[(size_t)s2 * n + me] / sizeof(neutral::ParticleRec));
  }
  ensure_capacity(g.send, out, out + out / 2 + 1024);
  ensure_capacity(g.recv, in, in + in / 2 + 1024);
  ensure_capacity(g.free_slots, (size_t)g.tiled_particles, (size_t)g.tiled_particles);
  /* the free list's length lives on the device next to the other exchange words */
  unsigned* d_nfree = g.d_exchange + 193;
  const unsigned nfree_now = (unsigned)g.mirror.holes();
  HIP_CHECK(hipMemcpyAsync(d_nfree, &nfree_now, sizeof(unsigned), hipMemcpyHostToDevice, g.stream));
  HIP_CHECK(hipMemcpyAsync(d_offsets, offsets, sizeof(unsigned) * (size_t)n, hipMemcpyHostToDevice,
                           g.stream));
  HIP_CHECK(neutral::launch_emigrant_pack(t, a.nparticles, g.domain, d_offsets, d_cursor, g.send.d,
                                          g.free_slots.d, d_nfree, g.stream));
  g.mirror.holes_changed((int)out);
  g.exchange_rounds++;
  g.emigrants += (unsigned long long)out;
  neutral::comm_exchange_bytes(g.send.d, g.recv.d, matrix, g.stream);
  g.host_syncs++;
  /* arrivals take the slots emigrants left first, then slots behind the records */
  const int reuse = ((int)in < g.mirror.holes()) ? (int)in : g.mirror.holes();
  const int grow = (int)in - reuse;
  if ((size_t)a.nparticles + (size_t)grow > (size_t)g.tiled_particles) {
    fprintf(stderr, "libneutral_hip: rank %d: %zu particles arrive but the store is full (%d "
                    "slots).\n", me, in, g.tiled_particles);
    exit(EXIT_FAILURE);
  }
  HIP_CHECK(neutral::launch_immigrant_append(t, g.recv.d, (int)in, a.nparticles, a.x_off, a.y_off,
                                             g.free_slots.d, g.mirror.holes(), reuse, g.stream));
  g.mirror.holes_changed(-reuse);
  return grow;
}

}  // namespace neutral_abi