/*
 * neutral_comb.hip -- the operations between two timesteps, on the SoA store
 * (include/neutral_hip.h): the census weight comb (neutral_hip_comb_particles), the fixed source
 * (neutral_hip_source_particles), the described source (neutral_hip_source_described), the mesh
 * source (neutral_hip_source_mesh) and the census
 * weight window (neutral_hip_window_particles), which rewrite the store; the census tally (neutral_hip_census_tally), which reads it into two meshes,
 * and the window bounds made from those (neutral_hip_window_bounds); the grouped forms of census
 * and window (neutral_hip_census_tally_groups, neutral_hip_window_particles_groups), a compile-time
 * parameter of their passes over the store, and their forms over blocks of cells
 * (neutral_hip_census_tally_blocks, neutral_hip_window_particles_blocks), a second one, with a
 * census pass that keeps few bins in LDS.  Beside them, on arrays of
 * doubles and no store at all, the batch statistics (neutral_hip_batch_fold,
 * neutral_hip_batch_statistics), which use the same reductions, header and decision.
 * What they share:
 *
 *   - the scan (scan<Op>): hierarchical, a tile of kCombTile elements per workgroup (kCombItems
 *     consecutive elements per lane, a wave64 shuffle scan of the lanes' totals, the four waves'
 *     totals through LDS), the tiles' sums scanned the same way one level up, and again if need
 *     be: three levels cover 2^33 elements.  A prefix sum is the sum of at most three levels' tile
 *     prefixes and one lane's running sum, some fifty additions deep whatever n: within 64 eps W of
 *     the exact sum.  Every combination is in a fixed order: the same input gives the same bits.
 *     What a scan reads and what its level 0 does with a prefix are policies (the *In and *Out
 *     structs): a prefix sum goes straight to its use and is never stored;
 *   - the workspace (Rooms): one allocation, handed out room by room; each operation's rooms are one
 *     struct, from which both its size and its pointers come;
 *   - header and decision: the kernels of a call tell each other and the host what they found
 *     through a header at the head of the workspace.  One thread decides (the header's `go`) and
 *     every later kernel returns at entry when it said no, so a call is enqueued without a wait and
 *     the host reads the header once (neutral_abi_store.hip: run_census_op);
 *   - the tile reduction (comb_reduce_tiles_kernel): the scans' way up, and, level upon level down
 *     to one value (reduce<Op>), what the census and the bounds know of a whole mesh.
 *
 * Each operation's own steps stand above its kernels.
 */
#include "neutral_device.h"
#include "neutral_inject.h"
#include "neutral_kernels.h"
#include "neutral_window_bins.h"

namespace neutral {

namespace {

struct SumF64 {
  using T = double;
  __device__ static T identity() { return 0.0; }
  __device__ static T op(T a, T b) { return a + b; }
};
struct MaxU32 {
  using T = unsigned;
  __device__ static T identity() { return 0u; }
  __device__ static T op(T a, T b) { return a > b ? a : b; }
};
struct SumU32 { /* (the fixed source's ranks: a count of at most n < 2^31) */
  using T = unsigned;
  __device__ static T identity() { return 0u; }
  __device__ static T op(T a, T b) { return a + b; }
};
struct SumU64 { /* (the window's demands: n * 63 does not fit 32 bits) */
  using T = unsigned long long;
  __device__ static T identity() { return 0ull; }
  __device__ static T op(T a, T b) { return a + b; }
};
struct OrU32 { /* (flags; reduced over a wave, never scanned) */
  using T = unsigned;
  __device__ static T identity() { return 0u; }
  __device__ static T op(T a, T b) { return a | b; }
};

/* the wave's 64 values combined, in lane 0: a tree, 32 down to 1 (a fixed order: an f64 sum keeps
 * its bits) */
template <class Op>
__device__ __forceinline__ typename Op::T wave_reduce(typename Op::T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    v = Op::op(v, __shfl_down(v, (unsigned)d, 64));
  }
  return v;
}

/* inclusive scan over the 64 lanes of a wave */
template <class Op>
__device__ __forceinline__ typename Op::T wave_inclusive(typename Op::T v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const typename Op::T below = __shfl_up(v, (unsigned)d, 64);
    if (lane >= d) {
      v = Op::op(below, v);
    }
  }
  return v;
}

/* the lanes' totals of a workgroup of kCombBlock -> what lies below this lane, and the
 * workgroup's total */
template <class Op>
__device__ __forceinline__ typename Op::T block_exclusive(typename Op::T total,
                                                          typename Op::T& block_total) {
  using T = typename Op::T;
  constexpr int kWaves = kCombBlock / 64;
  __shared__ T wave_total[kWaves];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)(threadIdx.x >> 6);
  const T inclusive = wave_inclusive<Op>(total);
  if (lane == 63) {
    wave_total[wave] = inclusive;
  }
  __syncthreads();
  T below_wave = Op::identity();
  T all = Op::identity();
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w == wave) {
      below_wave = all;
    }
    all = Op::op(all, wave_total[w]);
  }
  block_total = all;
  T below_lane = __shfl_up(inclusive, 1u, 64);
  if (lane == 0) {
    below_lane = Op::identity();
  }
  __syncthreads(); /* (wave_total is written again by the next call) */
  return Op::op(below_wave, below_lane);
}

/* the lanes' counts of a workgroup of kCombBlock added to *counter with one atomic (an integer: the
 * order the workgroups arrive in does not show); called by all lanes */
__device__ __forceinline__ void workgroup_count(unsigned mine, unsigned long long* counter) {
  constexpr int kWaves = kCombBlock / 64;
  __shared__ unsigned wave_count[kWaves];
  const unsigned of_wave = wave_reduce<SumU32>(mine);
  if ((threadIdx.x & 63u) == 0) {
    wave_count[threadIdx.x >> 6] = of_wave;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int v = 0; v < kWaves; ++v) {
      total += wave_count[v];
    }
    if (total) atomicAdd(counter, total);
  }
}

/* ---- what the scans read and write -------------------------------------------------- */

template <class T>
struct ArrayIn {
  const T* a;
  __device__ T load(long long j) const { return a[j]; }
};
template <class T>
struct ArrayOut {
  T* a;
  __device__ void store(long long j, T v, T /*total*/) { a[j] = v; }
  __device__ void finish() {}
};

struct LiveWeightIn {
  const double* weight;
  const int* dead;
  __device__ double load(long long j) const { return dead[j] == 0 ? weight[j] : 0.0; }
};

/* T(s): the teeth below s, #{k in 0..n-1 : fl(fl(k + v) * delta) < s}.  Monotone in s because
 * the tooth positions are non-decreasing in k; found from the quotient and set right by
 * comparing against the teeth themselves (a step or two). */
__device__ __forceinline__ unsigned teeth_below(double s, double v, double delta, long long n) {
  if (!(delta > 0.0) || !(delta <= 1.79769313486231570815e308) || !(s == s)) {
    return 0u; /* (no comb will run: CombHeader::go) */
  }
  double q = ceil(s / delta - v);
  q = (q > 0.0) ? q : 0.0; /* (a NaN lands here too) */
  q = (q < (double)n) ? q : (double)n;
  long long k = (long long)q;
  for (int i = 0; i < 4 && k > 0 && !(((double)(k - 1) + v) * delta < s); ++i) {
    --k;
  }
  for (int i = 0; i < 4 && k < n && ((double)k + v) * delta < s; ++i) {
    ++k;
  }
  return (unsigned)k;
}

/* level 0 of the weight scan: S_j goes straight into the tooth count */
struct TeethOut {
  const double* weight;
  const int* dead;
  unsigned* teeth;
  CombHeader* header;
  long long n;
  unsigned live = 0;
  unsigned bad = 0;
  __device__ void store(long long j, double s, double total) {
    const bool is_live = dead[j] == 0;
    if (is_live) {
      const double w = weight[j];
      live++;
      bad |= (!(w >= 0.0) || !(w <= 1.79769313486231570815e308)) ? 1u : 0u;
    }
    const double v = header->offset;
    const double delta = total / (double)n;
    teeth[j] = is_live ? teeth_below(s, v, delta, n) : 0u;
    if (j == n - 1) {
      header->weight = s; /* W = S_{n-1} */
    }
  }
  __device__ void finish() {
    /* one atomic per wave: integers, so the order they arrive in does not show */
    const unsigned l = wave_reduce<SumU32>(live), b = wave_reduce<OrU32>(bad);
    if ((threadIdx.x & 63u) == 0) {
      if (l) atomicAdd(&header->live, (unsigned long long)l);
      if (b) atomicOr(&header->bad, 1ull);
    }
  }
};

/* ---- the two kernels of a scan level ------------------------------------------------- */

/* sums[tile] = the tile's total */
template <class Op, class In>
__global__ __launch_bounds__(kCombBlock) void comb_reduce_tiles_kernel(In in, long long n,
                                                                        typename Op::T* sums) {
  using T = typename Op::T;
  const long long first = (long long)blockIdx.x * kCombTile + (long long)threadIdx.x * kCombItems;
  T total = Op::identity();
#pragma unroll
  for (int i = 0; i < kCombItems; ++i) {
    const long long j = first + i;
    total = Op::op(total, j < n ? in.load(j) : Op::identity());
  }
  T block_total;
  (void)block_exclusive<Op>(total, block_total);
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = block_total;
  }
}

/* out[j] = (what lies below the tile) + the inclusive scan inside it; tile_prefix: the
 * inclusive scan of the tiles' sums (null: one tile) */
template <class Op, class In, class Out>
__global__ __launch_bounds__(kCombBlock) void comb_scan_tiles_kernel(
    In in, long long n, const typename Op::T* tile_prefix, Out out) {
  using T = typename Op::T;
  const long long first = (long long)blockIdx.x * kCombTile + (long long)threadIdx.x * kCombItems;
  T running[kCombItems];
  T total = Op::identity();
#pragma unroll
  for (int i = 0; i < kCombItems; ++i) {
    const long long j = first + i;
    total = Op::op(total, j < n ? in.load(j) : Op::identity());
    running[i] = total;
  }
  T block_total;
  const T below_lane = block_exclusive<Op>(total, block_total);
  const T below_tile = (tile_prefix && blockIdx.x > 0) ? tile_prefix[blockIdx.x - 1] : Op::identity();
  const T everything = tile_prefix ? tile_prefix[gridDim.x - 1] : block_total;
  const T base = Op::op(below_tile, below_lane);
#pragma unroll
  for (int i = 0; i < kCombItems; ++i) {
    const long long j = first + i;
    if (j < n) {
      out.store(j, Op::op(base, running[i]), everything);
    }
  }
  out.finish();
}

unsigned tiles_of(long long n) { return (unsigned)((n + kCombTile - 1) / kCombTile); }

/* tile sums of every level above a scan of n elements */
size_t upper_level_elements(long long n) {
  size_t total = 0;
  while (n > kCombTile) {
    n = tiles_of(n);
    total += (size_t)n;
  }
  return total;
}

/* THE scan: out.store(j, the inclusive Op-scan of in.load(0 .. j), the total) for j in 0 .. n-1, one
 * out.finish() per lane.  Tile sums up, their scan in place (this function again, one level up),
 * and down.  `sums` has room for upper_level_elements(n) + 1 of Op::T */
template <class Op, class In, class Out>
hipError_t scan(In in, long long n, typename Op::T* sums, Out out, hipStream_t stream) {
  using T = typename Op::T;
  const unsigned tiles = tiles_of(n);
  if (tiles > 1) {
    hipLaunchKernelGGL((comb_reduce_tiles_kernel<Op, In>), dim3(tiles), dim3(kCombBlock), 0, stream, in,
                       n, sums);
    if (hipError_t e = scan<Op>(ArrayIn<T>{sums}, (long long)tiles, sums + tiles, ArrayOut<T>{sums},
                                stream)) {
      return e;
    }
  }
  hipLaunchKernelGGL((comb_scan_tiles_kernel<Op, In, Out>), dim3(tiles), dim3(kCombBlock), 0, stream,
                     in, n, tiles > 1 ? (const T*)sums : (const T*)nullptr, out);
  return hipGetLastError();
}

/* inclusive scan of data[0..n) in place */
template <class Op>
hipError_t scan_in_place(typename Op::T* data, long long n, typename Op::T* sums, hipStream_t stream) {
  return scan<Op>(ArrayIn<typename Op::T>{data}, n, sums, ArrayOut<typename Op::T>{data}, stream);
}

/* ---- the workspace ---------------------------------------------------------------------
 * One allocation, handed out room by room at multiples of 256 bytes.  Every operation has one struct
 * of its rooms, filled in one fixed order with the header first (run_census_op reads the header from
 * the head); its *_workspace_bytes function builds that struct over a null base, which only counts,
 * and its launcher builds it over the allocation: size and pointers come from the same lines. */
constexpr size_t align_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

class Rooms {
 public:
  explicit Rooms(void* base) : base_((char*)base) {}
  template <class T>
  T* take(size_t count) {
    T* room = base_ ? (T*)(base_ + bytes_) : nullptr;
    bytes_ += align_up(sizeof(T) * count);
    return room;
  }
  size_t bytes() const { return bytes_; }

 private:
  char* base_;
  size_t bytes_ = 0;
};

/* what an operation's rooms come to */
template <class OpRooms, class... Sizes>
size_t bytes_of(Sizes... sizes) {
  Rooms r(nullptr);
  const OpRooms rooms(r, sizes...);
  (void)rooms;
  return r.bytes();
}

size_t at_least_one(long long n) { return (size_t)(n > 0 ? n : 1); }
/* the tile sums of a scan or a reduction over n elements */
size_t sums_elements(long long n) { return upper_level_elements(n) + 1; }

struct CombRooms {
  CombHeader* header;
  double* scratch; /* the gather's; the two cell indexes go through it as one int2 */
  unsigned* teeth;
  unsigned* src;
  double* sums; /* (the u32 scans use the same room) */
  CombRooms(Rooms& r, long long n)
      : header(r.take<CombHeader>(1)), scratch(r.take<double>(at_least_one(n))),
        teeth(r.take<unsigned>(at_least_one(n))), src(r.take<unsigned>(at_least_one(n))),
        sums(r.take<double>(sums_elements(n))) {}
};

/* what the three sources share: the refilled slots in rank order and the tile sums of their scan */
template <class Header>
struct SourceRooms {
  Header* header;
  unsigned* list;
  unsigned* sums;
  SourceRooms(Rooms& r, long long n)
      : header(r.take<Header>(1)), list(r.take<unsigned>(at_least_one(n))),
        sums(r.take<unsigned>(sums_elements(n))) {}
};
struct DescribedRooms : SourceRooms<DescribedSourceHeader> {
  DescribedTables* tables;
  DescribedRooms(Rooms& r, long long n) : SourceRooms(r, n), tables(r.take<DescribedTables>(1)) {}
};
struct MeshSourceRooms : SourceRooms<MeshSourceHeader> {
  MeshSourceBins* bins;
  double* cumulative; /* C_c of the K non-zero cells, in cell order */
  unsigned* rank;     /* every cell's rank among the non-zero ones */
  unsigned* cell_of;  /* the cell at every rank */
  double* mesh_sums;  /* of the scans over the cells (the u32 scan uses the same room) */
  MeshSourceRooms(Rooms& r, long long n, long long cells)
      : SourceRooms(r, n), bins(r.take<MeshSourceBins>(1)), cumulative(r.take<double>(at_least_one(cells))),
        rank(r.take<unsigned>(at_least_one(cells))), cell_of(r.take<unsigned>(at_least_one(cells))),
        mesh_sums(r.take<double>(sums_elements(cells))) {}
};

template <class Header>
struct WindowRoomsOf {
  Header* header;
  double* new_weight; /* of every source */
  unsigned* list;     /* the free slots, ascending */
  unsigned* owner;    /* of every granted request */
  unsigned long long* sums; /* (the u32 scans use the same room) */
  unsigned char* code;      /* the verdict on every slot */
  WindowRoomsOf(Rooms& r, long long n)
      : header(r.take<Header>(1)), new_weight(r.take<double>(at_least_one(n))),
        list(r.take<unsigned>(at_least_one(n))), owner(r.take<unsigned>(at_least_one(n))),
        sums(r.take<unsigned long long>(sums_elements(n))), code(r.take<unsigned char>(at_least_one(n))) {}
};
using WindowRooms = WindowRoomsOf<WindowHeader>;
struct GroupWindowRooms : WindowRoomsOf<GroupWindowHeader> {
  double* edges; /* the G + 1 group edges */
  GroupWindowRooms(Rooms& r, long long n)
      : WindowRoomsOf(r, n), edges(r.take<double>(kSpectrumMaxGroups + 1)) {}
};

/* the two mesh operations: header and mesh are neighbours (the census clears both at once), the flag
 * stands behind the mesh (one all-reduce sums mesh and flag) */
struct CensusRooms {
  static constexpr int kReductions = 4;
  union Header {
    CensusHeader census;
    GroupCensusHeader groups; /* (the census's, one counter longer) */
    BoundsHeader bounds;
  };
  size_t cells;
  Header* header;
  double* mesh; /* 2 * cells doubles and the flag */
  double* sums[kReductions];
  CensusRooms(Rooms& r, int nx, int ny)
      : cells(at_least_one(nx) * at_least_one(ny)), header(r.take<Header>(1)),
        mesh(r.take<double>(mesh_doubles())) {
    for (double*& s : sums) {
      s = r.take<double>(sums_elements((long long)cells));
    }
  }
  size_t mesh_doubles() const { return 2 * cells + 1; }
};
/* the grouped census: G meshes back to back are one mesh of nx by G * ny, so every room scales with
 * G; the edges stand behind them */
struct GroupCensusRooms : CensusRooms {
  double* edges;
  GroupCensusRooms(Rooms& r, int nx, int ny, int ngroups)
      : CensusRooms(r, nx, ngroups * ny), edges(r.take<double>(kSpectrumMaxGroups + 1)) {}
};

struct BatchRooms {
  static constexpr int kReductions = 6;
  BatchHeader* header;
  double* sums[kReductions];
  BatchRooms(Rooms& r, long long len) : header(r.take<BatchHeader>(1)) {
    for (double*& s : sums) {
      s = r.take<double>(sums_elements(at_least_one(len)));
    }
  }
};

/* ---- the comb's own kernels ----------------------------------------------------------- */

__global__ void comb_begin_kernel(CombHeader* h, uint64_t pkey, uint64_t seed) {
  double rn0, rn1;
  generate_random_numbers(pkey, seed, 0, rn0, rn1);
  h->offset = 1.0 - rn0;
  h->weight = 0.0;
  h->weight_each = 0.0;
  h->live = 0;
  h->bad = 0;
  h->sources = 0;
  h->max_copies = 0;
  h->go = 0;
}

__global__ void comb_decide_kernel(CombHeader* h, long long n) {
  const double w = h->weight;
  const bool ok = h->live > 0 && h->bad == 0 && w > 0.0 && w <= 1.79769313486231570815e308;
  h->weight_each = ok ? w / (double)n : 0.0;
  h->go = ok ? 1ull : 0ull;
}

__global__ __launch_bounds__(kCombBlock) void comb_clear_kernel(const CombHeader* h, unsigned* src,
                                                                long long n) {
  if (!h->go) return;
  const long long k = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k < n) {
    src[k] = 0u;
  }
}

/* every particle that owns teeth writes its index at the first of them */
__global__ __launch_bounds__(kCombBlock) void comb_heads_kernel(CombHeader* h, const unsigned* teeth,
                                                                unsigned* src, long long n) {
  if (!h->go) return;
  unsigned sources = 0, most = 0;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < n;
       j += (long long)gridDim.x * kCombBlock) {
    const unsigned end = teeth[j];
    const unsigned begin = j > 0 ? teeth[j - 1] : 0u;
    if (end > begin) { /* (begin < end <= n: inside src[]) */
      src[begin] = (unsigned)j;
      sources++;
      most = (end - begin > most) ? end - begin : most;
    }
  }
  sources = wave_reduce<SumU32>(sources);
  most = wave_reduce<MaxU32>(most);
  if ((threadIdx.x & 63u) == 0 && sources) {
    atomicAdd(&h->sources, (unsigned long long)sources);
    atomicMax(&h->max_copies, (unsigned long long)most);
  }
}

template <class T>
__global__ __launch_bounds__(kCombBlock) void comb_gather_kernel(const CombHeader* h, const T* field,
                                                                 const unsigned* src, T* scratch,
                                                                 long long n) {
  if (!h->go) return;
  const long long k = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k < n) {
    scratch[k] = field[src[k]];
  }
}

/* the two cell indexes share a pass: both fit the scratch of n doubles */
__global__ __launch_bounds__(kCombBlock) void comb_gather_cells_kernel(const CombHeader* h,
                                                                       const int* cellx, const int* celly,
                                                                       const unsigned* src, int2* scratch,
                                                                       long long n) {
  if (!h->go) return;
  const long long k = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k < n) {
    const unsigned j = src[k];
    scratch[k] = make_int2(cellx[j], celly[j]);
  }
}

template <class T>
__global__ __launch_bounds__(kCombBlock) void comb_copy_back_kernel(const CombHeader* h, const T* scratch,
                                                                    T* field, long long n) {
  if (!h->go) return;
  const long long k = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k < n) {
    field[k] = scratch[k];
  }
}

/* cellx, celly from the scratch; every slot alive at W / n */
__global__ __launch_bounds__(kCombBlock) void comb_finish_kernel(const CombHeader* h, const int2* scratch,
                                                                 int* cellx, int* celly, double* weight,
                                                                 int* dead, long long n) {
  if (!h->go) return;
  const long long k = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k < n) {
    const int2 c = scratch[k];
    cellx[k] = c.x;
    celly[k] = c.y;
    weight[k] = h->weight_each;
    dead[k] = 0;
  }
}

/* ---- the fixed source (include/neutral_hip.h: neutral_hip_source_particles) -------------
 * An inclusive sum-scan of the dead flags gives every dead slot j its rank r_j = 1, 2, ... in
 * ascending index order; the slots of rank <= count are refilled. */

struct DeadIn {
  const int* dead;
  __device__ unsigned load(long long j) const { return dead[j] != 0 ? 1u : 0u; }
};

/* level 0 of the rank scan: the slot of every rank that is refilled
 * goes into list[rank - 1] (ascending, so the fill's lanes are dense and its stores ordered);
 * the lane of the last slot fills the header */
struct SourceListOut {
  const int* dead;
  unsigned* list;
  SourceHeader* header;
  long long n;
  unsigned count;
  __device__ void store(long long j, unsigned rank, unsigned total) {
    if (dead[j] != 0 && rank <= count) { /* (1 <= rank <= min(count, total) <= n: inside list[]) */
      list[rank - 1] = (unsigned)j;
    }
    if (j == n - 1) {
      header->dead = total;
      header->emitted = total < count ? total : count;
    }
  }
  __device__ void finish() {}
};

/* one lane per refilled slot, in rank order */
__global__ __launch_bounds__(kCombBlock) void source_fill_kernel(InjectArgs a, const SourceHeader* h,
                                                                 const unsigned* list, uint64_t seed,
                                                                 double weight) {
  const unsigned long long r = (unsigned long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (r < h->emitted) {
    inject_slot(a, (int)list[r], seed, weight, plain_source(a));
  }
}

/* ---- the described source (include/neutral_hip.h: neutral_hip_source_described) ----------
 * The fixed source's scan and list; the fill draws counter 2 of the slot's stream first and walks
 * the two tables of cumulative shares with it: which component, which of its energy bins.  The
 * tables are read by every lane at an index of its own, so a workgroup stages what is in use of
 * them in LDS once (at most 16 * 72 + 256 * 24 bytes) and then takes trip after trip of ranks. */
constexpr unsigned kDescribedFillBlocks = 2048; /* (eight workgroups for each of 256 CUs) */
__global__ __launch_bounds__(kCombBlock) void described_fill_kernel(InjectArgs a, DescribedSourceHeader* h,
                                                                    const unsigned* list,
                                                                    const DescribedTables* tables,
                                                                    int ncomponents, int nbins,
                                                                    uint64_t seed, double weight) {
  const unsigned long long emitted = h->base.emitted;
  if ((unsigned long long)blockIdx.x * kCombBlock >= emitted) {
    return; /* (the whole workgroup: the grid is sized by count, not by the dead) */
  }
  constexpr int kWaves = kCombBlock / 64;
  __shared__ DescribedTables t;
  __shared__ unsigned counts[kWaves][kDescribedMaxComponents];
  {
    static_assert(sizeof(DescribedComponent) % 8 == 0 && sizeof(DescribedBin) % 8 == 0, "copied as words");
    constexpr int kComponentWords = (int)(sizeof(DescribedComponent) / 8);
    constexpr int kBinWords = (int)(sizeof(DescribedBin) / 8);
    const unsigned long long* from = (const unsigned long long*)tables->components;
    unsigned long long* to = (unsigned long long*)t.components;
    for (int i = (int)threadIdx.x; i < ncomponents * kComponentWords; i += kCombBlock) {
      to[i] = from[i];
    }
    from = (const unsigned long long*)tables->bins;
    to = (unsigned long long*)t.bins;
    for (int i = (int)threadIdx.x; i < nbins * kBinWords; i += kCombBlock) {
      to[i] = from[i];
    }
    if (threadIdx.x < (unsigned)(kWaves * kDescribedMaxComponents)) {
      (&counts[0][0])[threadIdx.x] = 0u;
    }
  }
  __syncthreads();

  /* trip after trip of gridDim.x * kCombBlock consecutive ranks (the trip count is the
   * workgroup's: the ballots below see whole waves) */
  for (unsigned long long first = (unsigned long long)blockIdx.x * kCombBlock; first < emitted;
       first += (unsigned long long)gridDim.x * kCombBlock) {
    const unsigned long long r = first + threadIdx.x;
    int mine = -1; /* the component this lane's slot comes out of */
    if (r < emitted) {
      const int slot = (int)list[r];
      double u0, u1;
      generate_random_numbers(a.pid_base + (uint64_t)slot, seed, 2, u0, u1);
      /* the first component with t < C_k, else the last (u0 lies in (0, 1]: t == S happens) */
      const double at = u0 * t.components[ncomponents - 1].cumulative;
      int k = 0;
      while (k < ncomponents - 1 && !(at < t.components[k].cumulative)) {
        ++k;
      }
      const DescribedComponent& c = t.components[k];
      /* ... and the first of its bins with tb < B_{k,b}, else its last */
      const double at_bin = u1 * c.bin_total;
      int b = c.bin_first;
      const int last = c.bin_first + c.bin_count - 1; /* (inside bins[]: the host checked the range) */
      double below = t.bins[b].share; /* B_{k,b}: the host's running sum, the same additions */
      while (b < last && !(at_bin < below)) {
        ++b;
        below += t.bins[b].share;
      }
      inject_slot(a, slot, seed, weight,
                  SlotSource{c.left, c.bottom, c.width, c.height, c.theta0, c.theta_width, t.bins[b].e_lo,
                             t.bins[b].e_hi});
      mine = k;
    }
    /* the wave's count of every component by ballot, kept in the wave's own row of LDS */
    for (int c = 0; c < ncomponents; ++c) {
      const unsigned in_wave = (unsigned)__popcll(__ballot(mine == c));
      if ((threadIdx.x & 63u) == 0 && in_wave) {
        counts[threadIdx.x >> 6][c] += in_wave;
      }
    }
  }
  /* one atomic per workgroup and component, from at most kDescribedFillBlocks workgroups: integers,
   * so the order they arrive in does not show.  (With a workgroup per 256 slots, 39 000 atomics on
   * one word for 1e7 slots out of one component, the call took 0.60 ms against the fixed source's
   * 0.33: profiles/described_source.) */
  __syncthreads();
  if (threadIdx.x < (unsigned)ncomponents) {
    unsigned total = 0;
    for (int v = 0; v < kWaves; ++v) {
      total += counts[v][threadIdx.x];
    }
    if (total) {
      atomicAdd(&h->by_component[threadIdx.x], (unsigned long long)total);
    }
  }
}

/* ---- the mesh source (include/neutral_hip.h: neutral_hip_source_mesh) ---------------------
 *   1. the fixed source's scan and list of the dead slots;
 *   2. an inclusive u32 sum-scan of "strength > 0" over the cells: every cell's rank among the K
 *      non-zero ones; its level 0 looks at every strength and raises the flag at one that is negative
 *      or not finite;
 *   3. the f64 sum-scan of the strengths (what is not > 0 counts as 0.0); its level 0 stores C_c and c
 *      at rank - 1 of every non-zero cell, and the last cell's lane S;
 *   4. one thread decides (MeshSourceHeader::go); the fill returns at entry when it said no;
 *   5. the fill, one lane per refilled slot, trip after trip of ranks as the described source's:
 *      counter 2 of the slot's stream, a bisection of the K cumulative sums for the first with
 *      t < C, else the last -- a cell of strength 0 has no entry and cannot be chosen --, the walk
 *      over the bins, inject_slot with the cell's box and the cell itself.
 * The table is read by every lane at places of its own, 8 * K bytes that sit in L2.  With
 * NEUTRAL_MESH_SOURCE_COARSE a workgroup stages every q-th entry, q = ceil(K / kMeshCoarseEntries),
 * in LDS once (at most 16 KB): the top levels of every bisection then cost no memory trip and
 * log2(q) probes of the table are left.  Both forms give the same cell wherever the table ascends
 * (profiles/mesh_source/README.md has their times). */
#ifndef NEUTRAL_MESH_SOURCE_COARSE
#define NEUTRAL_MESH_SOURCE_COARSE 1
#endif
constexpr bool kMeshCoarse = NEUTRAL_MESH_SOURCE_COARSE != 0;
constexpr unsigned kMeshCoarseEntries = 2048;
/* a cap on the grid, not what is resident: with 22.5 KB of LDS and 106 VGPRs four workgroups fit a CU,
 * so 2 048 of them run in about two rounds on 256 CUs; each stages the coarse table once and then
 * takes trip after trip of ranks */
constexpr unsigned kMeshFillBlocks = 2048;

struct StrengthPositiveIn {
  const double* strength;
  __device__ unsigned load(long long c) const { return strength[c] > 0.0 ? 1u : 0u; }
};
struct StrengthIn { /* (a NaN or a negative entry counts as 0.0 here: the call is refused for it) */
  const double* strength;
  __device__ double load(long long c) const {
    const double s = strength[c];
    return s > 0.0 ? s : 0.0;
  }
};

/* level 0 of the rank scan: rank[c], the flag, and K from the lane of the last cell */
struct MeshRankOut {
  const double* strength;
  unsigned* rank;
  MeshSourceHeader* header;
  long long cells;
  unsigned bad = 0;
  __device__ void store(long long c, unsigned r, unsigned total) {
    const double s = strength[c];
    bad |= (!(s >= 0.0) || !(s <= 1.79769313486231570815e308)) ? 1u : 0u;
    rank[c] = r;
    if (c == cells - 1) {
      header->nonzero = total;
    }
  }
  __device__ void finish() {
    const unsigned b = wave_reduce<OrU32>(bad);
    if ((threadIdx.x & 63u) == 0 && b) {
      atomicOr(&header->bad, 1ull);
    }
  }
};

/* level 0 of the strength scan: C_c and c at the rank of every non-zero cell (1 <= rank <= K <=
 * cells: inside both arrays); S = C of the last cell */
struct MeshCumulativeOut {
  const double* strength;
  const unsigned* rank;
  double* cumulative;
  unsigned* cell_of;
  MeshSourceHeader* header;
  long long cells;
  __device__ void store(long long c, double sum, double /*total*/) {
    if (strength[c] > 0.0) {
      const unsigned r = rank[c] - 1u;
      cumulative[r] = sum;
      cell_of[r] = (unsigned)c;
    }
    if (c == cells - 1) {
      header->total = sum;
    }
  }
  __device__ void finish() {}
};

__global__ void mesh_source_decide_kernel(MeshSourceHeader* h) {
  const double s = h->total;
  const bool ok = h->bad == 0 && h->nonzero > 0 && s > 0.0 && s <= 1.79769313486231570815e308;
  h->go = ok ? 1ull : 0ull;
}

template <bool kCoarse>
__global__ __launch_bounds__(kCombBlock) void mesh_fill_kernel(InjectArgs a, const MeshSourceHeader* h,
                                                               const unsigned* list,
                                                               const double* __restrict__ cumulative,
                                                               const unsigned* __restrict__ cell_of,
                                                               const MeshSourceBins* bins, MeshSourceArgs m,
                                                               uint64_t seed, double weight) {
  if (!h->go) return;
  const unsigned long long emitted = h->base.emitted;
  if ((unsigned long long)blockIdx.x * kCombBlock >= emitted) {
    return; /* (the whole workgroup: the grid is sized by count, not by the dead) */
  }
  const unsigned nonzero = (unsigned)h->nonzero; /* K >= 1: the decision saw to it */
  const double total = h->total;
  __shared__ DescribedBin bin[kDescribedMaxBins];
  __shared__ double coarse[kCoarse ? kMeshCoarseEntries : 1];
  /* entry i of the coarse table is C at place min((i + 1) * every, K) - 1: the last of its run */
  const unsigned every = kCoarse ? (nonzero + kMeshCoarseEntries - 1) / kMeshCoarseEntries : 1u;
  const unsigned ncoarse = kCoarse ? (nonzero + every - 1) / every : 0u; /* (<= kMeshCoarseEntries) */
  {
    static_assert(sizeof(DescribedBin) % 8 == 0, "copied as words");
    constexpr int kBinWords = (int)(sizeof(DescribedBin) / 8);
    const unsigned long long* from = (const unsigned long long*)bins->bins;
    unsigned long long* to = (unsigned long long*)bin;
    for (int i = (int)threadIdx.x; i < m.nbins * kBinWords; i += kCombBlock) {
      to[i] = from[i];
    }
    for (unsigned i = threadIdx.x; i < ncoarse; i += kCombBlock) {
      const unsigned long long at = (unsigned long long)(i + 1u) * every;
      coarse[i] = cumulative[(at < nonzero ? at : nonzero) - 1u];
    }
  }
  __syncthreads();

  const double* edgex = a.edgex + a.pad;
  const double* edgey = a.edgey + a.pad;
  for (unsigned long long r = (unsigned long long)blockIdx.x * kCombBlock + threadIdx.x; r < emitted;
       r += (unsigned long long)gridDim.x * kCombBlock) {
    const int slot = (int)list[r];
    double u0, u1;
    generate_random_numbers(a.pid_base + (uint64_t)slot, seed, 2, u0, u1);
    /* the first place with t < C, else the last (u0 lies in (0, 1]: t == S happens) */
    const double at = __dmul_rn(u0, total);
    unsigned lo = 0, hi = nonzero - 1u;
    if (kCoarse) {
      unsigned clo = 0, chi = ncoarse - 1u;
      while (clo < chi) {
        const unsigned mid = (clo + chi) >> 1;
        if (at < coarse[mid]) {
          chi = mid;
        } else {
          clo = mid + 1u;
        }
      }
      lo = clo * every; /* (clo < ncoarse: lo < K) */
      hi = (nonzero - lo > every ? lo + every : nonzero) - 1u;
    }
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (at < cumulative[mid]) {
        hi = mid;
      } else {
        lo = mid + 1u;
      }
    }
    const unsigned c = cell_of[lo]; /* (< cells: a cell's own index) */
    const int i = (int)(c % (unsigned)a.local_nx), j = (int)(c / (unsigned)a.local_nx);
    /* ... and the first bin with tb < B_b, else the last: the described source's walk */
    const double at_bin = __dmul_rn(u1, m.bin_total);
    int b = 0;
    double below = bin[0].share;
    while (b < m.nbins - 1 && !(at_bin < below)) {
      ++b;
      below += bin[b].share;
    }
    const double left = edgex[i], bottom = edgey[j];
    inject_slot(a, slot, seed, weight,
                SlotSource{left, bottom, edgex[i + 1] - left, edgey[j + 1] - bottom, m.theta0, m.theta_width,
                           bin[b].e_lo, bin[b].e_hi},
                GivenCell{a.x_off + i, a.y_off + j});
  }
}

/* ---- the bank source (include/neutral_hip.h: neutral_hip_source_bank) ---------------------
 *   1. the fixed source's scan and list of the dead slots;
 *   2. one lane per slot that would be refilled looks at its record (rank k: records[first + k]) and
 *      keeps the lowest bad index in the header (an atomic min by the lanes that found one: rare);
 *   3. the fill, as many lanes, returns at entry when there is one; else the record as four 16-byte
 *      loads, the shift, the snap, the cell, the eleven fields through the arrays.
 * Every operation on a coordinate or a weight is one IEEE operation by intrinsic: nothing contracts. */
struct BankRecordWords {
  double x, y, omega_x, omega_y, energy, weight, time_left;
  unsigned slot, side;
};
__device__ __forceinline__ BankRecordWords load_bank_record(const EscapeRecord* r) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d* in = (const v2d*)r;
  const v2d w0 = in[0], w1 = in[1], w2 = in[2], w3 = in[3];
  BankRecordWords o;
  o.x = w0.x;
  o.y = w0.y;
  o.omega_x = w1.x;
  o.omega_y = w1.y;
  o.energy = w2.x;
  o.weight = w2.y;
  o.time_left = w3.x;
  o.slot = (unsigned)__double2loint(w3.y);
  o.side = (unsigned)__double2hiint(w3.y);
  return o;
}
__device__ __forceinline__ bool bank_finite(double v) {
  return v >= -1.79769313486231570815e308 && v <= 1.79769313486231570815e308;
}
/* a shifted coordinate against its axis: -> 0 inside [lo, hi]; 1 moved onto a wall (p is the wall);
 * 2 outside by more than snap (or not a number) */
__device__ __forceinline__ int bank_snap(double& p, double lo, double hi, double snap) {
  const double under = __dsub_rn(lo, p), over = __dsub_rn(p, hi);
  if (under > 0.0) {
    if (!(under <= snap)) return 2;
    p = lo;
    return 1;
  }
  if (over > 0.0) {
    if (!(over <= snap)) return 2;
    p = hi;
    return 1;
  }
  return (p >= lo && p <= hi) ? 0 : 2;
}
/* the largest c in [0, n - 1] with edge[c] <= p (lo <= p <= hi); on an edge and moving down: the cell below */
__device__ __forceinline__ int bank_cell(const double* __restrict__ edge, int n, double p, double omega) {
  int lo = 0, hi = n; /* edge[lo] <= p; hi == n or p < edge[hi] */
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p < edge[mid]) {
      hi = mid;
    } else {
      lo = mid;
    }
  }
  return (p == edge[lo] && omega < 0.0 && lo > 0) ? lo - 1 : lo;
}

__global__ void bank_begin_kernel(BankSourceHeader* h) {
  h->first_bad = ~0ull;
  h->snapped = 0;
  h->weight = 0.0;
}

__global__ __launch_bounds__(kCombBlock) void bank_check_kernel(InjectArgs a, BankSourceHeader* h, BankSourceArgs b) {
  const unsigned long long k = (unsigned long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (k >= h->base.emitted) {
    return;
  }
  const BankRecordWords r = load_bank_record(b.records + b.first + k);
  bool bad = r.side > 3u || !bank_finite(r.x) || !bank_finite(r.y) || !bank_finite(r.omega_x) ||
             !bank_finite(r.omega_y) || !bank_finite(r.energy) || !bank_finite(r.weight) ||
             !bank_finite(r.time_left) || !(r.weight > 0.0) || !(r.energy > 0.0) ||
             (r.omega_x == 0.0 && r.omega_y == 0.0);
  if (!bad) {
    double x = __dadd_rn(r.x, b.shift[2 * r.side]), y = __dadd_rn(r.y, b.shift[2 * r.side + 1]);
    const double* ex = a.edgex + a.pad;
    const double* ey = a.edgey + a.pad;
    bad = bank_snap(x, ex[0], ex[a.local_nx], b.snap) == 2 || bank_snap(y, ey[0], ey[a.local_ny], b.snap) == 2;
  }
  if (bad) {
    atomicMin(&h->first_bad, b.first + k);
  }
}

__global__ __launch_bounds__(kCombBlock) void bank_fill_kernel(InjectArgs a, BankSourceHeader* h,
                                                               const unsigned* list, BankSourceArgs b) {
  if (h->first_bad != ~0ull) {
    return; /* (a record the call refuses: nothing is written) */
  }
  const unsigned long long k = (unsigned long long)blockIdx.x * kCombBlock + threadIdx.x;
  unsigned moved = 0;
  double written = 0.0;
  if (k < h->base.emitted) {
    const BankRecordWords r = load_bank_record(b.records + b.first + k);
    const int side = (int)(r.side & 3u);
    double x = __dadd_rn(r.x, b.shift[2 * side]), y = __dadd_rn(r.y, b.shift[2 * side + 1]);
    const double* ex = a.edgex + a.pad;
    const double* ey = a.edgey + a.pad;
    moved = (bank_snap(x, ex[0], ex[a.local_nx], b.snap) == 1 ? 1u : 0u) +
            (bank_snap(y, ey[0], ey[a.local_ny], b.snap) == 1 ? 1u : 0u);
    const int slot = (int)list[k];
    written = __dmul_rn(r.weight, b.weight_scale);
    a.p.x[slot] = x;
    a.p.y[slot] = y;
    a.p.cellx[slot] = a.x_off + bank_cell(ex, a.local_nx, x, r.omega_x);
    a.p.celly[slot] = a.y_off + bank_cell(ey, a.local_ny, y, r.omega_y);
    a.p.omega_x[slot] = r.omega_x;
    a.p.omega_y[slot] = r.omega_y;
    a.p.energy[slot] = r.energy;
    a.p.weight[slot] = written;
    a.p.dt_to_census[slot] = a.dt;
    a.p.mfp_to_collision[slot] = 0.0;
    a.p.dead[slot] = 0;
  }
  /* (whole waves reach here: the two sums per wave, one atomic each from its first lane) */
  const unsigned wave_moved = wave_reduce<SumU32>(moved);
  const double wave_written = wave_reduce<SumF64>(written);
  if ((threadIdx.x & 63u) == 0) {
    if (wave_moved) {
      atomicAdd(&h->snapped, (unsigned long long)wave_moved);
    }
    if (wave_written != 0.0) {
      atomicAdd(&h->weight, wave_written);
    }
  }
}

/* ---- the census weight window (include/neutral_hip.h: neutral_hip_window_particles) ------
 *   1. the classification: the one pass over the store (dead, weight, cellx, celly: 20 bytes per
 *      slot, the gather of lower[], the roulette draw of a slot under its bound).  What it found
 *      goes into one byte per slot, so that the scans and roulette's stores read that byte;
 *   2. an inclusive u32 sum-scan of "free" (dead going in, or killed just now): list[rank - 1] = j;
 *   3. one thread decides (WindowHeader::go); every later kernel returns at entry when it said no;
 *   4. an inclusive u64 sum-scan of the demands e_j; its level 0 knows D_j and F, hence g_j: it
 *      writes the head owner[D_j] = j and the new weight w / (1 + g_j) into the workspace;
 *   5. the comb's running maximum over owner[0 .. granted): indices ascend;
 *   6. roulette's stores, then one lane per granted request copies owner[r] into list[r]; the
 *      first lane of a source rewrites the source's own weight, which no other lane reads (the
 *      copies take the new weight from the workspace).
 * granted is known on the device alone: the kernels of 5 are launched for n and their In / Out
 * touch no memory beyond it. */

enum : unsigned char {
  kWindowKeep = 0,     /* live, inside its window or in a cell without one */
  kWindowDead = 1,     /* dead going in */
  kWindowKilled = 2,   /* roulette: lost */
  kWindowSurvived = 3, /* roulette: goes on at w_s */
  kWindowDemand = 4    /* + (e_j - 1), e_j = m - 1 in 1 .. 63: the codes 4 .. 66 */
};

/* ---- energy groups: the compile-time parameter of the window's and the census's pass over the
 * store (include/neutral_hip.h: neutral_hip_window_particles_groups) -------------------------
 * A policy says how many meshes stand back to back and which of them a slot's energy chooses.
 * NoGroups is the plain calls': one mesh, no energy read, nothing counted -- not an instruction of
 * the other form is left in their kernels. */
struct NoGroups {
  static constexpr bool kOn = false;
  struct Staged {};
  __device__ Staged stage() const { return Staged{}; }
  __device__ long long meshes() const { return 1; }
};
struct EnergyGroups {
  static constexpr bool kOn = true;
  const double* edges;         /* [device] ngroups + 1, ascending */
  int ngroups;                 /* 1 .. kSpectrumMaxGroups */
  unsigned long long* outside; /* the header's counter of live slots in no group */
  struct Staged {
    const double* edges; /* the workgroup's copy in LDS */
  };
  /* once per workgroup, by all of its lanes */
  __device__ Staged stage() const {
    __shared__ double staged[kSpectrumMaxGroups + 1];
    for (int i = (int)threadIdx.x; i <= ngroups; i += kCombBlock) {
      staged[i] = edges[i];
    }
    __syncthreads();
    return Staged{staged};
  }
  __device__ long long meshes() const { return ngroups; }
  /* (group_of_edges, neutral_window_bins.h: on an edge the group above; -1 outside) */
  __device__ int group_of(const double* e, double energy) const { return group_of_edges(e, ngroups, energy); }
};

/* ---- blocks of cells: the second compile-time parameter of the same passes (include/neutral_hip.h:
 * neutral_hip_window_particles_blocks) -----------------------------------------------------------
 * A policy says on what mesh the bins lie and which of its cells a checked cell falls into.
 * UnitCells is the plain and the grouped calls': the transport mesh itself, every function the
 * identity -- their kernels keep their instructions.  BlockCells is a coarse mesh of cnx by cny
 * blocks of block_x by block_y cells, the last of a row or column perhaps narrower.
 * The division by a block's edge is BlockDivisor's (neutral_window_bins.h). */
struct UnitCells {
  static constexpr bool kOn = false;
  __device__ int nx(int nx) const { return nx; }
  __device__ int ny(int ny) const { return ny; }
  __device__ int x(int cellx) const { return cellx; }
  __device__ int y(int celly) const { return celly; }
};
struct BlockCells {
  static constexpr bool kOn = true;
  int cnx, cny; /* ceil(nx / block_x), ceil(ny / block_y) */
  BlockDivisor by_x, by_y;
  __device__ int nx(int) const { return cnx; }
  __device__ int ny(int) const { return cny; }
  __device__ int x(int cellx) const { return by_x.quotient(cellx); }
  __device__ int y(int celly) const { return by_y.quotient(celly); }
};

/* the verdict on slot j (kWindow...); refuse: a live slot the call does not accept.  Every f64
 * operation is one IEEE operation, in the order of the header's definition.  Grouped: a live slot
 * that passed the checks and lies in no group has no window (outside goes up by one); the others
 * look their bound up in their group's mesh.  Blocks: the check is on the true cell, the bound the
 * block's. */
template <class Groups, class Cells>
__device__ __forceinline__ unsigned window_classify(const ParticleView& p, const WindowArgs& a,
                                                    const Groups& groups,
                                                    const typename Groups::Staged& staged,
                                                    const Cells& cells, long long j,
                                                    bool& refuse, double& w, double& w_s,
                                                    unsigned& outside) {
  constexpr double kMax = 1.79769313486231570815e308;
  w = 0.0;
  w_s = 0.0;
  if (p.dead[j] != 0) {
    return kWindowDead;
  }
  const int cx = p.cellx[j], cy = p.celly[j];
  w = p.weight[j];
  double energy = 0.0;
  if constexpr (Groups::kOn) {
    energy = p.energy[j]; /* (goes out with the three loads above) */
  }
  if ((unsigned)cx >= (unsigned)a.nx || (unsigned)cy >= (unsigned)a.ny || !(w >= 0.0) || !(w <= kMax)) {
    refuse = true;
    return kWindowKeep;
  }
  long long bin = (long long)cells.y(cy) * cells.nx(a.nx) + cells.x(cx);
  if constexpr (Groups::kOn) {
    const int g = groups.group_of(staged.edges, energy);
    if (g < 0) {
      outside++;
      return kWindowKeep;
    }
    bin += (long long)g * cells.ny(a.ny) * cells.nx(a.nx); /* (< G * ny * nx: inside lower[]) */
  }
  const double w_lo = a.lower[bin];
  if (!(w_lo >= 0.0) || !(w_lo <= kMax)) {
    refuse = true;
    return kWindowKeep;
  }
  if (w_lo == 0.0) {
    return kWindowKeep; /* no window in this cell */
  }
  if (w < w_lo) {
    double rn0, rn1;
    generate_random_numbers(a.pid_base + (uint64_t)j, a.seed, 0, rn0, rn1);
    w_s = __dmul_rn(a.survival_ratio, w_lo);
    return __dmul_rn(rn0, w_s) < w ? kWindowSurvived : kWindowKilled;
  }
  const double w_hi = __dmul_rn(a.upper_ratio, w_lo);
  if (w > w_hi) {
    const double c = ceil(__ddiv_rn(w, w_hi));
    const int m = c >= (double)a.max_split ? a.max_split : (int)c;
    return m >= 2 ? kWindowDemand + (unsigned)(m - 2) : kWindowKeep;
  }
  return kWindowKeep;
}

template <class Header>
__global__ void window_begin_kernel(Header* h) {
  *h = Header{};
}

template <class Groups, class Cells>
__global__ __launch_bounds__(kCombBlock) void window_classify_kernel(ParticleView p, WindowArgs a,
                                                                     unsigned char* code,
                                                                     WindowHeader* h, long long n,
                                                                     Groups groups, Cells cells) {
  const typename Groups::Staged staged = groups.stage();
  unsigned dead = 0, live = 0, killed = 0, survived = 0, above = 0, bad = 0, outside = 0;
  unsigned long long demand = 0;
  double lost = 0.0, gained = 0.0;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < n;
       j += (long long)gridDim.x * kCombBlock) {
    bool refuse = false;
    double w, w_s;
    const unsigned c = window_classify(p, a, groups, staged, cells, j, refuse, w, w_s, outside);
    code[j] = (unsigned char)c;
    bad |= refuse ? 1u : 0u;
    dead += c == kWindowDead ? 1u : 0u;
    live += c != kWindowDead ? 1u : 0u;
    if (c == kWindowKilled) {
      killed++;
      lost += w;
    } else if (c == kWindowSurvived) {
      survived++;
      gained += w_s - w;
    } else if (c >= kWindowDemand) {
      above++;
      demand += c - kWindowDemand + 1u;
    }
  }
  /* one atomic per workgroup and counter, all on one line of the header: with one per wave the
   * call took 0.93 ms at 1e6 slots, most of it these atomics queueing, and 0.12 ms with this
   * ("The census weight window").  Integers, so the order they arrive in
   * does not show (the two weight sums are f64: they depend on it in their last bits) */
  constexpr int kWaves = kCombBlock / 64;
  __shared__ unsigned long long counts[kWaves][7];
  __shared__ double weights[kWaves][2];
  const unsigned long long mine[7] = {
      wave_reduce<SumU32>(dead),  wave_reduce<SumU32>(live), wave_reduce<SumU32>(killed), wave_reduce<SumU32>(survived),
      wave_reduce<SumU32>(above), wave_reduce<SumU32>(bad),  wave_reduce<SumU64>(demand)};
  lost = wave_reduce<SumF64>(lost);
  gained = wave_reduce<SumF64>(gained);
  if ((threadIdx.x & 63u) == 0) {
    for (int k = 0; k < 7; ++k) {
      counts[threadIdx.x >> 6][k] = mine[k];
    }
    weights[threadIdx.x >> 6][0] = lost;
    weights[threadIdx.x >> 6][1] = gained;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total[7] = {0, 0, 0, 0, 0, 0, 0};
    double w[2] = {0.0, 0.0};
    for (int v = 0; v < kWaves; ++v) { /* (a fixed order) */
      for (int k = 0; k < 7; ++k) {
        total[k] += counts[v][k];
      }
      w[0] += weights[v][0];
      w[1] += weights[v][1];
    }
    if (total[0]) atomicAdd(&h->dead, total[0]);
    if (total[1]) atomicAdd(&h->live, total[1]);
    if (total[2]) atomicAdd(&h->killed, total[2]);
    if (total[3]) atomicAdd(&h->survived, total[3]);
    if (total[4]) atomicAdd(&h->above, total[4]);
    if (total[5]) atomicOr(&h->bad, 1ull);
    if (total[6]) atomicAdd(&h->demand, total[6]);
    if (total[2]) atomicAdd(&h->lost, w[0]);
    if (total[3]) atomicAdd(&h->gained, w[1]);
  }
  if constexpr (Groups::kOn) {
    workgroup_count(outside, groups.outside);
  }
}

struct WindowFreeIn {
  const unsigned char* code;
  __device__ unsigned load(long long j) const {
    const unsigned c = code[j];
    return (c == kWindowDead || c == kWindowKilled) ? 1u : 0u;
  }
};

/* level 0 of the free-rank scan: list[rank - 1] = j (1 <= rank <= F <= n: inside list[]) */
struct WindowListOut {
  const unsigned char* code;
  unsigned* list;
  WindowHeader* header;
  long long n;
  __device__ void store(long long j, unsigned rank, unsigned total) {
    const unsigned c = code[j];
    if (c == kWindowDead || c == kWindowKilled) {
      list[rank - 1] = (unsigned)j;
    }
    if (j == n - 1) {
      header->free_slots = total;
    }
  }
  __device__ void finish() {}
};

__global__ void window_decide_kernel(WindowHeader* h) {
  const bool ok = h->bad == 0;
  h->granted = ok ? (h->demand < h->free_slots ? h->demand : h->free_slots) : 0ull;
  h->go = ok ? 1ull : 0ull;
}

__global__ __launch_bounds__(kCombBlock) void window_clear_kernel(const WindowHeader* h, unsigned* owner) {
  if (!h->go) return;
  const long long granted = (long long)h->granted; /* (<= F <= n: inside owner[]) */
  for (long long r = (long long)blockIdx.x * kCombBlock + threadIdx.x; r < granted;
       r += (long long)gridDim.x * kCombBlock) {
    owner[r] = 0u;
  }
}

struct WindowDemandIn {
  const unsigned char* code;
  __device__ unsigned long long load(long long j) const {
    const unsigned c = code[j];
    return c >= kWindowDemand ? (unsigned long long)(c - kWindowDemand + 1u) : 0ull;
  }
};

/* level 0 of the demand scan: D_j = (inclusive sum) - e_j; a demander with D_j < F is granted
 * g_j = min(e_j, F - D_j) >= 1 copies: its head goes to owner[D_j] (D_j < granted: inside the part
 * that was cleared) and its new weight into the workspace */
struct WindowHeadsOut {
  const unsigned char* code;
  const double* weight;
  unsigned* owner;
  double* new_weight;
  WindowHeader* header;
  unsigned split = 0;
  __device__ void store(long long j, unsigned long long inclusive, unsigned long long /*total*/) {
    const unsigned c = code[j];
    if (c >= kWindowDemand && header->go) {
      const unsigned long long e = c - kWindowDemand + 1u;
      const unsigned long long below = inclusive - e;
      const unsigned long long supply = header->free_slots;
      if (below < supply) {
        const unsigned long long g = supply - below < e ? supply - below : e;
        owner[below] = (unsigned)j;
        new_weight[j] = __ddiv_rn(weight[j], (double)(1ull + g));
        split++;
      }
    }
  }
  __device__ void finish() {
    const unsigned s = wave_reduce<SumU32>(split);
    if ((threadIdx.x & 63u) == 0 && s) {
      atomicAdd(&header->split, (unsigned long long)s);
    }
  }
};

/* owner[0 .. granted), for scan kernels launched over n: nothing beyond it is read or written */
struct WindowOwnerIn {
  const unsigned* owner;
  const WindowHeader* header;
  __device__ unsigned load(long long r) const {
    return (unsigned long long)r < header->granted ? owner[r] : 0u;
  }
};
struct WindowOwnerOut {
  unsigned* owner;
  const WindowHeader* header;
  __device__ void store(long long r, unsigned v, unsigned /*total*/) {
    if ((unsigned long long)r < header->granted) {
      owner[r] = v;
    }
  }
  __device__ void finish() {}
};

/* roulette's stores: before the fill, which may hand a slot freed here to a copy.  Grouped: a
 * survivor's group is worked out again -- its energy is what the classification saw, so it lies in
 * a group -- with the edges read where they stand: survivors are few and a workgroup may have none */
template <class Groups, class Cells>
__global__ __launch_bounds__(kCombBlock) void window_roulette_kernel(ParticleView p, WindowArgs a,
                                                                     const unsigned char* code,
                                                                     const WindowHeader* h, long long n,
                                                                     Groups groups, Cells cells) {
  if (!h->go || h->killed + h->survived == 0) return;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < n;
       j += (long long)gridDim.x * kCombBlock) {
    const unsigned c = code[j];
    if (c == kWindowKilled) {
      p.dead[j] = 1;
      p.weight[j] = 0.0;
    } else if (c == kWindowSurvived) {
      long long bin = (long long)cells.y(p.celly[j]) * cells.nx(a.nx) + cells.x(p.cellx[j]);
      if constexpr (Groups::kOn) {
        const int g = groups.group_of(groups.edges, p.energy[j]);
        if (g < 0) continue; /* (cannot happen; and nothing is read outside lower[] if it does) */
        bin += (long long)g * cells.ny(a.ny) * cells.nx(a.nx);
      }
      const double w_lo = a.lower[bin]; /* (checked by the classification) */
      p.weight[j] = __dmul_rn(a.survival_ratio, w_lo);
    }
  }
}

/* one lane per granted request r: slot list[r] becomes a copy of owner[r] at the source's new
 * weight.  Destinations are distinct free slots and no free slot is a source. */
__global__ __launch_bounds__(kCombBlock) void window_fill_kernel(ParticleView p, const WindowHeader* h,
                                                                 const unsigned* owner,
                                                                 const unsigned* list,
                                                                 const double* new_weight) {
  if (!h->go) return;
  const long long granted = (long long)h->granted;
  for (long long r = (long long)blockIdx.x * kCombBlock + threadIdx.x; r < granted;
       r += (long long)gridDim.x * kCombBlock) {
    const unsigned j = owner[r];
    const unsigned k = list[r];
    const double w = new_weight[j];
    p.x[k] = p.x[j];
    p.y[k] = p.y[j];
    p.omega_x[k] = p.omega_x[j];
    p.omega_y[k] = p.omega_y[j];
    p.energy[k] = p.energy[j];
    p.dt_to_census[k] = p.dt_to_census[j];
    p.mfp_to_collision[k] = p.mfp_to_collision[j];
    p.cellx[k] = p.cellx[j];
    p.celly[k] = p.celly[j];
    p.weight[k] = w;
    p.dead[k] = 0;
    if (r == 0 || owner[r - 1] != j) {
      p.weight[j] = w; /* (the source's own: nobody reads it in this kernel) */
    }
  }
}

/* ---- the census tally (include/neutral_hip.h: neutral_hip_census_tally) -----------------
 *   1. header and mesh zeroed; the one pass over the store (dead, cellx, celly, weight: 20 bytes
 *      per slot): a live lane adds 1.0 and its weight to its cell with two no-return f64 atomics; a
 *      live slot the call refuses adds nothing and raises the flag, which then stands behind the
 *      mesh as one more double (several ranks: one all-reduce sums mesh and flag);
 *   2. four reductions over the cells (comb_reduce_tiles_kernel, level upon level): occupied cells
 *      and the largest count (counts in doubles: exact), the weight and the largest cell's weight;
 *   3. one thread decides (CensusHeader::go); one lane per cell writes the caller's two meshes, or
 *      zeros.
 * Where a lane's two adds go is the one difference between the two forms measured
 * (profiles/census/README.md): two meshes of `cells` doubles, the adds 8 * cells bytes apart, or
 * {count, weight} pairs, both adds in one 16-byte segment.  Step 3 reads either. */
#ifndef NEUTRAL_CENSUS_PAIRS
#define NEUTRAL_CENSUS_PAIRS 0
#endif
constexpr bool kCensusPairs = NEUTRAL_CENSUS_PAIRS != 0;

__device__ __forceinline__ long long census_count_at(long long c, long long cells) {
  return kCensusPairs ? 2 * c : c;
}
__device__ __forceinline__ long long census_weight_at(long long c, long long cells) {
  return kCensusPairs ? 2 * c + 1 : cells + c;
}

struct MaxF64 { /* (of values that are not negative) */
  using T = double;
  __device__ static T identity() { return 0.0; }
  __device__ static T op(T a, T b) { return a > b ? a : b; }
};

/* the Op-combination of in.load(0 .. n-1): tile sums, theirs one level up, down to one value; ->
 * where it will stand.  `sums` has room for upper_level_elements(n) + 1 of Op::T */
template <class Op, class In>
const typename Op::T* reduce(In in, long long n, typename Op::T* sums, hipStream_t stream) {
  using T = typename Op::T;
  const unsigned tiles = tiles_of(n);
  hipLaunchKernelGGL((comb_reduce_tiles_kernel<Op, In>), dim3(tiles), dim3(kCombBlock), 0, stream, in, n,
                     sums);
  return tiles == 1 ? sums : reduce<Op>(ArrayIn<T>{sums}, (long long)tiles, sums + tiles, stream);
}

/* ---- where a live lane's two adds go: the third compile-time parameter of the census's pass ----
 * GlobalBins is the form above: two no-return f64 atomics per live lane into the workspace's mesh.
 * On few bins that collapses (24 ns per live slot on one bin: every add of the chip queues on two
 * addresses).  LdsBins sums on chip what shares a destination before the global add: the workgroup
 * keeps the bins in dynamic LDS -- `bins` doubles for the weights, then `bins` u32 for the counts,
 * 12 bytes a bin --, a live lane adds there (ds_add_u32: exact; ds_add_f64 under the build's
 * -munsafe-fp-atomics, as the stream kernel's tally window has it), and after a barrier the
 * workgroup flushes its non-empty bins with one global add each for (double)count and the weight.
 * Every workgroup starts its flush kCombBlock bins further on than the one before it (mod bins):
 * where the bins outnumber a workgroup's lanes, the workgroups that finish together do not queue
 * on the same rows.  Counts below 2^31 per workgroup; the sums of the counts are whole numbers in
 * doubles, exact in any order, and the weights' sum is the other form's up to the order of its
 * additions. */
struct GlobalBins {
  double* mesh;
  struct Staged {};
  __device__ Staged stage(long long) const { return Staged{}; }
  __device__ void add(const Staged&, long long c, long long bins, double w) const {
    atomicAdd(&mesh[census_count_at(c, bins)], 1.0);
    atomicAdd(&mesh[census_weight_at(c, bins)], w);
  }
  __device__ void flush(const Staged&, long long) const {}
};
struct LdsBins {
  double* mesh;
  struct Staged {
    double* weight;
    unsigned* count;
  };
  /* once per workgroup, by all of its lanes; bins <= kCensusLdsBinsMax */
  __device__ Staged stage(long long bins) const {
    extern __shared__ double census_lds[];
    const Staged s{census_lds, (unsigned*)(census_lds + bins)};
    for (int b = (int)threadIdx.x; b < (int)bins; b += kCombBlock) {
      s.weight[b] = 0.0;
      s.count[b] = 0u;
    }
    __syncthreads();
    return s;
  }
  __device__ void add(const Staged& s, long long c, long long, double w) const {
    atomicAdd(&s.count[c], 1u);
    atomicAdd(&s.weight[c], w);
  }
  __device__ void flush(const Staged& s, long long bins) const {
    __syncthreads();
    const int first = (int)((blockIdx.x * (unsigned)kCombBlock) % (unsigned)bins); /* (once per workgroup) */
    for (int i = (int)threadIdx.x; i < (int)bins; i += kCombBlock) {
      const int b = i + first < (int)bins ? i + first : i + first - (int)bins;
      const unsigned count = s.count[b];
      if (count != 0u) {
        atomicAdd(&mesh[census_count_at(b, bins)], (double)count);
        atomicAdd(&mesh[census_weight_at(b, bins)], s.weight[b]);
      }
    }
  }
};

/* (grouped: `bins` counts the bins of all G meshes, a slot's energy goes out with its other loads,
 * and a live slot in no group is checked, counted in live and outside, and scores nowhere; blocks:
 * the check is on the true cell, the bin the block's) */
template <class Groups, class Cells, class Bins>
__global__ __launch_bounds__(kCombBlock) void census_score_kernel(ParticleView p, int nx, int ny,
                                                                  Bins sink, CensusHeader* h,
                                                                  long long n, Groups groups,
                                                                  Cells blocks) {
  constexpr double kMax = 1.79769313486231570815e308;
  const typename Groups::Staged staged = groups.stage();
  const long long cells = (long long)blocks.nx(nx) * blocks.ny(ny) * groups.meshes();
  const typename Bins::Staged bins = sink.stage(cells);
  unsigned live = 0, dead = 0, bad = 0, outside = 0;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < n;
       j += (long long)gridDim.x * kCombBlock) {
    /* (the four loads go out together; a dead slot's three other words are never looked at) */
    const int is_dead = p.dead[j];
    const int cx = p.cellx[j], cy = p.celly[j];
    const double w = p.weight[j];
    double energy = 0.0;
    if constexpr (Groups::kOn) {
      energy = p.energy[j];
    }
    if (is_dead != 0) {
      dead++;
      continue;
    }
    live++;
    if ((unsigned)cx >= (unsigned)nx || (unsigned)cy >= (unsigned)ny || !(w >= 0.0) || !(w <= kMax)) {
      bad = 1u;
      continue;
    }
    /* (0 <= c < cells: inside both forms of the mesh) */
    long long c = (long long)blocks.y(cy) * blocks.nx(nx) + blocks.x(cx);
    if constexpr (Groups::kOn) {
      const int g = groups.group_of(staged.edges, energy);
      if (g < 0) {
        outside++;
        continue;
      }
      c += (long long)g * blocks.ny(ny) * blocks.nx(nx);
    }
    sink.add(bins, c, cells, w);
  }
  sink.flush(bins, cells);
  /* one atomic per workgroup and counter, as the window's classification has them */
  constexpr int kWaves = kCombBlock / 64;
  __shared__ unsigned counts[kWaves][3];
  const unsigned mine[3] = {wave_reduce<SumU32>(live), wave_reduce<SumU32>(dead), wave_reduce<OrU32>(bad)};
  if ((threadIdx.x & 63u) == 0) {
    for (int k = 0; k < 3; ++k) {
      counts[threadIdx.x >> 6][k] = mine[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total[3] = {0, 0, 0};
    for (int v = 0; v < kWaves; ++v) {
      total[0] += counts[v][0];
      total[1] += counts[v][1];
      total[2] |= counts[v][2];
    }
    if (total[0]) atomicAdd(&h->live, total[0]);
    if (total[1]) atomicAdd(&h->dead, total[1]);
    if (total[2]) atomicOr(&h->bad, 1ull);
  }
  if constexpr (Groups::kOn) {
    workgroup_count(outside, groups.outside);
  }
}

/* the flag, behind the mesh: what the all-reduce over the ranks carries of a refusal */
__global__ void census_flag_kernel(const CensusHeader* h, double* flag) { *flag = h->bad ? 1.0 : 0.0; }

struct CensusCountIn {
  const double* mesh;
  long long cells;
  __device__ double load(long long c) const { return mesh[census_count_at(c, cells)]; }
};
struct CensusOccupiedIn {
  const double* mesh;
  long long cells;
  __device__ double load(long long c) const { return mesh[census_count_at(c, cells)] > 0.0 ? 1.0 : 0.0; }
};
struct CensusWeightIn {
  const double* mesh;
  long long cells;
  __device__ double load(long long c) const { return mesh[census_weight_at(c, cells)]; }
};

__global__ void census_decide_kernel(CensusHeader* h, const double* flag, const double* occupied,
                                     const double* max_count, const double* weight,
                                     const double* max_weight) {
  const bool ok = *flag == 0.0;
  h->occupied = ok ? (unsigned long long)*occupied : 0ull; /* (whole numbers below 2^53: exact) */
  h->max_count = ok ? (unsigned long long)*max_count : 0ull;
  h->weight = ok ? *weight : 0.0;
  h->max_cell_weight = ok ? *max_weight : 0.0;
  h->go = ok ? 1ull : 0ull;
}

/* one lane per cell: the caller's two meshes from either form of the workspace's, or zeros */
__global__ __launch_bounds__(kCombBlock) void census_fill_kernel(const CensusHeader* h, const double* mesh,
                                                                 double* out, long long cells) {
  const long long c = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  if (c < cells) {
    const bool go = h->go != 0;
    out[c] = go ? mesh[census_count_at(c, cells)] : 0.0;
    out[cells + c] = go ? mesh[census_weight_at(c, cells)] : 0.0;
  }
}

/* ---- the window bounds (include/neutral_hip.h: neutral_hip_window_bounds) ------------------
 * Three reductions over the census the caller hands in (K, M, and whether an entry is negative
 * or not finite), one thread's decision and peak, one lane per cell.  Every f64 operation is one
 * IEEE operation, in the order of the header's definition. */
__device__ __forceinline__ bool bounds_eligible(const BoundsArgs& a, long long c, double& w) {
  const long long cells = (long long)a.nx * a.ny;
  w = a.census[cells + c];
  return a.census[c] >= (double)a.min_count && w > 0.0;
}
struct BoundsEligibleIn {
  BoundsArgs a;
  __device__ double load(long long c) const {
    double w;
    return bounds_eligible(a, c, w) ? 1.0 : 0.0;
  }
};
struct BoundsWeightIn {
  BoundsArgs a;
  __device__ double load(long long c) const {
    double w;
    return bounds_eligible(a, c, w) ? w : 0.0;
  }
};
struct BoundsBadIn { /* a cell's two entries */
  const double* census;
  long long cells;
  __device__ double load(long long c) const {
    constexpr double kMax = 1.79769313486231570815e308;
    const double count = census[c], w = census[cells + c];
    return (!(count >= 0.0) || !(count <= kMax) || !(w >= 0.0) || !(w <= kMax)) ? 1.0 : 0.0;
  }
};

__global__ void bounds_decide_kernel(BoundsHeader* h, BoundsArgs a, const double* eligible,
                                     const double* max_weight, const double* bad) {
  const unsigned long long k = (unsigned long long)*eligible; /* (a whole number below 2^53: exact) */
  const double m = *max_weight;
  const bool ok = *bad == 0.0 && k > 0;
  const double twice = __dmul_rn(2.0, (double)k);
  const double above = __dmul_rn(twice, m);
  const double below = __dmul_rn(__dadd_rn(1.0, a.upper_ratio), a.target_population);
  h->eligible = ok ? k : 0ull;
  h->floored = 0ull;
  h->bad = *bad != 0.0 ? 1ull : 0ull;
  h->max_cell_weight = ok ? m : 0.0;
  h->peak = ok ? __ddiv_rn(above, below) : 0.0;
  h->go = ok ? 1ull : 0ull;
}

__global__ __launch_bounds__(kCombBlock) void bounds_fill_kernel(BoundsHeader* h, BoundsArgs a,
                                                                 double* lower_out) {
  if (!h->go) return;
  const long long cells = (long long)a.nx * a.ny;
  const long long c = (long long)blockIdx.x * kCombBlock + threadIdx.x;
  unsigned floored = 0;
  if (c < cells) {
    double w;
    double lower = 0.0; /* no window in this cell */
    if (bounds_eligible(a, c, w)) {
      const double r = __ddiv_rn(w, h->max_cell_weight);
      floored = r < a.floor_ratio ? 1u : 0u;
      lower = __dmul_rn(fmax(r, a.floor_ratio), h->peak);
    }
    lower_out[c] = lower;
  }
  floored = wave_reduce<SumU32>(floored);
  if ((threadIdx.x & 63u) == 0 && floored) {
    atomicAdd(&h->floored, (unsigned long long)floored);
  }
}

/* ---- batch statistics (include/neutral_hip.h: neutral_hip_batch_fold,
 * neutral_hip_batch_statistics) ----------------------------------------------------------
 * Both work on an array of doubles and know nothing of what it is a tally of.  Each has one pass
 * that checks (a reduction: is an entry not usable?), one thread's decision (BatchHeader::go), and
 * one elementwise, grid-strided pass that writes -- or returns at entry.  Every f64 operation is
 * one IEEE operation in the order of the header's definition: the functions below are kept out
 * of contraction, so that a product is rounded before it is added. */
constexpr int kBatchMaxBlocks = 4096; /* the elementwise passes are grid-strided */
constexpr double kBatchMax = 1.79769313486231570815e308;

__device__ __forceinline__ bool batch_finite(double v) { return v >= -kBatchMax && v <= kBatchMax; }

struct BatchNotFiniteIn {
  const double* x;
  __device__ double load(long long j) const { return batch_finite(x[j]) ? 0.0 : 1.0; }
};
struct BatchNonzeroIn { /* (a count held in a double: exact) */
  const double* x;
  __device__ double load(long long j) const { return x[j] != 0.0 ? 1.0 : 0.0; }
};
struct BatchBadMomentsIn { /* an entry's mean and M2 */
  const double* moments;
  long long len;
  __device__ double load(long long j) const {
    const double m2 = moments[len + j];
    return (batch_finite(moments[j]) && m2 >= 0.0 && m2 <= kBatchMax) ? 0.0 : 1.0;
  }
};
struct BatchWithinIn { /* a scored entry whose relerr is at most the limit */
  const double* moments;
  const double* relerr;
  double limit;
  __device__ double load(long long j) const { return (moments[j] != 0.0 && relerr[j] <= limit) ? 1.0 : 0.0; }
};
struct BatchScoredRelerrIn {
  const double* moments;
  const double* relerr;
  __device__ double load(long long j) const { return moments[j] != 0.0 ? relerr[j] : 0.0; }
};

/* Welford's update of one entry with batch number k > 1 */
__device__ __forceinline__ void batch_welford(double x, double k, double& mean, double& m2) {
#pragma clang fp contract(off)
  const double d = x - mean;
  const double step = d / k;
  const double next = mean + step;
  const double d2 = x - next;
  const double product = d * d2;
  mean = next;
  m2 = m2 + product;
}

/* estimate and relerr of one entry from its moments, B batches */
__device__ __forceinline__ void batch_entry(double mean, double m2, double scale, double b,
                                            double& estimate, double& relerr) {
#pragma clang fp contract(off)
  estimate = scale * mean;
  const double var = m2 / (b - 1.0); /* (b - 1.0: a whole number, exact) */
  const double se = __dsqrt_rn(var / b);
  relerr = mean != 0.0 ? se / fabs(mean) : 0.0;
}

__global__ void batch_fold_decide_kernel(BatchHeader* h, const double* bad, const double* sum,
                                         const double* nonzero) {
  const bool ok = *bad == 0.0;
  *h = BatchHeader{};
  h->bad = ok ? 0ull : 1ull;
  h->sum = ok ? *sum : 0.0;
  h->nonzero = ok ? (unsigned long long)*nonzero : 0ull; /* (a whole number below 2^53: exact) */
  h->go = ok ? 1ull : 0ull;
}

__global__ __launch_bounds__(kCombBlock) void batch_fold_kernel(const BatchHeader* h, const double* x,
                                                                long long len, int k, double* moments) {
  if (!h->go) return;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < len;
       j += (long long)gridDim.x * kCombBlock) {
    const double v = x[j];
    double mean = v, m2 = 0.0;
    if (k > 1) { /* (k == 1: what moments held is never read) */
      mean = moments[j];
      m2 = moments[len + j];
      batch_welford(v, (double)k, mean, m2);
    }
    moments[j] = mean;
    moments[len + j] = m2;
  }
}

__global__ void batch_stats_decide_kernel(BatchHeader* h, const double* bad) {
  const bool ok = *bad == 0.0;
  *h = BatchHeader{};
  h->bad = ok ? 0ull : 1ull;
  h->go = ok ? 1ull : 0ull;
}

__global__ __launch_bounds__(kCombBlock) void batch_stats_kernel(const BatchHeader* h, const double* moments,
                                                                 long long len, int nbatches, double scale,
                                                                 double* estimate_out, double* relerr_out) {
  if (!h->go) return;
  for (long long j = (long long)blockIdx.x * kCombBlock + threadIdx.x; j < len;
       j += (long long)gridDim.x * kCombBlock) {
    double estimate, relerr;
    batch_entry(moments[j], moments[len + j], scale, (double)nbatches, estimate, relerr);
    estimate_out[j] = estimate;
    relerr_out[j] = relerr;
  }
}

/* (a refused call's reductions ran over whatever the outputs held: nothing of them is kept) */
__global__ void batch_stats_finish_kernel(BatchHeader* h, const double* scored, const double* within10,
                                          const double* within5, const double* max_relerr,
                                          const double* relerr_sum, const double* estimate_sum) {
  if (!h->go) return;
  h->scored = (unsigned long long)*scored; /* (whole numbers below 2^53: exact) */
  h->within10 = (unsigned long long)*within10;
  h->within5 = (unsigned long long)*within5;
  h->max_relerr = *max_relerr;
  h->relerr_sum = *relerr_sum;
  h->mean_relerr = *scored > 0.0 ? __ddiv_rn(*relerr_sum, *scored) : 0.0;
  h->sum = *estimate_sum;
}

unsigned batch_blocks(long long len) {
  const long long blocks = (len + kCombBlock - 1) / kCombBlock;
  return (unsigned)(blocks < kBatchMaxBlocks ? blocks : kBatchMaxBlocks);
}

}  // namespace

size_t batch_workspace_bytes(size_t len) { return bytes_of<BatchRooms>((long long)len); }

hipError_t launch_batch_fold(const double* x, size_t len, int k, double* moments, void* workspace,
                             hipStream_t stream) {
  const long long n = (long long)len;
  Rooms r(workspace);
  const BatchRooms ws(r, n);
  const double* bad = reduce<MaxF64>(BatchNotFiniteIn{x}, n, ws.sums[0], stream);
  const double* sum = reduce<SumF64>(ArrayIn<double>{x}, n, ws.sums[1], stream);
  const double* nonzero = reduce<SumF64>(BatchNonzeroIn{x}, n, ws.sums[2], stream);
  hipLaunchKernelGGL(batch_fold_decide_kernel, dim3(1), dim3(1), 0, stream, ws.header, bad, sum, nonzero);
  hipLaunchKernelGGL(batch_fold_kernel, dim3(batch_blocks(n)), dim3(kCombBlock), 0, stream,
                     (const BatchHeader*)ws.header, x, n, k, moments);
  return hipGetLastError();
}

hipError_t launch_batch_statistics(const double* moments, size_t len, int nbatches, double scale,
                                   double* estimate_out, double* relerr_out, void* workspace,
                                   hipStream_t stream) {
  const long long n = (long long)len;
  Rooms r(workspace);
  const BatchRooms ws(r, n);
  BatchHeader* header = ws.header;
  const double* bad = reduce<MaxF64>(BatchBadMomentsIn{moments, n}, n, ws.sums[0], stream);
  hipLaunchKernelGGL(batch_stats_decide_kernel, dim3(1), dim3(1), 0, stream, header, bad);
  hipLaunchKernelGGL(batch_stats_kernel, dim3(batch_blocks(n)), dim3(kCombBlock), 0, stream,
                     (const BatchHeader*)header, moments, n, nbatches, scale, estimate_out, relerr_out);
  const double* scored = reduce<SumF64>(BatchNonzeroIn{moments}, n, ws.sums[0], stream);
  const double* within10 = reduce<SumF64>(BatchWithinIn{moments, relerr_out, 0.1}, n, ws.sums[1], stream);
  const double* within5 = reduce<SumF64>(BatchWithinIn{moments, relerr_out, 0.05}, n, ws.sums[2], stream);
  const double* max_relerr = reduce<MaxF64>(BatchScoredRelerrIn{moments, relerr_out}, n, ws.sums[3], stream);
  const double* relerr_sum = reduce<SumF64>(BatchScoredRelerrIn{moments, relerr_out}, n, ws.sums[4], stream);
  const double* estimate_sum = reduce<SumF64>(ArrayIn<double>{estimate_out}, n, ws.sums[5], stream);
  hipLaunchKernelGGL(batch_stats_finish_kernel, dim3(1), dim3(1), 0, stream, header, scored, within10, within5,
                     max_relerr, relerr_sum, estimate_sum);
  return hipGetLastError();
}

size_t census_workspace_bytes(int nx, int ny) { return bytes_of<CensusRooms>(nx, ny); }
double* census_mesh(void* workspace) {
  Rooms r(workspace);
  return CensusRooms(r, 1, 1).mesh; /* (where the mesh begins does not depend on the cells) */
}
size_t census_mesh_doubles(int nx, int ny) {
  Rooms r(nullptr);
  return CensusRooms(r, nx, ny).mesh_doubles();
}

namespace {

/* whether the pass keeps its bins in LDS (the blocks census decides, launch_census_score_blocks) */
struct CensusLds {
  bool on = false;
  int compute_units = 0;
};
size_t census_lds_bytes(long long bins) { return (size_t)bins * (sizeof(double) + sizeof(unsigned)); }

/* the first half of any census: ws is the rooms of all the meshes, nx by ny the transport mesh */
template <class Groups, class Cells>
hipError_t census_score(const ParticleView& p, long long n, int nx, int ny, const CensusRooms& ws,
                        Groups groups, Cells blocks, hipStream_t stream, const CensusLds& lds = CensusLds{}) {
  CensusHeader* header = &ws.header->census;
  /* (a tile's worth of slots per workgroup at least, kCensusMaxBlocks workgroups at most) */
  const unsigned tiles = tiles_of(n);
  if (tiles > 0) { /* (an empty shard among several ranks' scores nothing: its zeros go into the sum) */
    bool in_lds = false;
    if constexpr (Cells::kOn) { /* (the LDS form is the blocks census's alone) */
      if (lds.on) {
        /* the workgroups that are resident at once and no more -- every one of them flushes its
         * bins, and a workgroup that starts late only adds a flush.  A CU holds 160 KB of LDS (the
         * bins, and at most 1 KB of the kernel's own) and eight workgroups of four waves */
        const size_t bytes = census_lds_bytes((long long)ws.cells);
        const size_t fit = (size_t)(160 * 1024) / (bytes + 1024);
        const unsigned per_cu = (unsigned)(fit < 1 ? 1 : fit > 8 ? 8 : fit);
        const unsigned resident = (unsigned)(lds.compute_units > 0 ? lds.compute_units : 256) * per_cu;
        hipLaunchKernelGGL((census_score_kernel<Groups, Cells, LdsBins>),
                           dim3(tiles < resident ? tiles : resident), dim3(kCombBlock), bytes, stream, p, nx, ny,
                           LdsBins{ws.mesh}, header, n, groups, blocks);
        in_lds = true;
      }
    }
    if (!in_lds) {
      hipLaunchKernelGGL((census_score_kernel<Groups, Cells, GlobalBins>),
                         dim3(tiles < (unsigned)kCensusMaxBlocks ? tiles : (unsigned)kCensusMaxBlocks),
                         dim3(kCombBlock), 0, stream, p, nx, ny, GlobalBins{ws.mesh}, header, n, groups, blocks);
    }
  }
  hipLaunchKernelGGL(census_flag_kernel, dim3(1), dim3(1), 0, stream, (const CensusHeader*)header,
                     ws.mesh + 2 * ws.cells);
  return hipGetLastError();
}

/* (header and mesh are neighbours: one clear) */
hipError_t census_clear(const CensusRooms& ws, void* workspace, hipStream_t stream) {
  return hipMemsetAsync(workspace, 0, (size_t)((char*)(ws.mesh + ws.mesh_doubles()) - (char*)workspace), stream);
}

}  // namespace

hipError_t launch_census_score(const ParticleView& p, int nparticles, int nx, int ny, void* workspace,
                               hipStream_t stream) {
  Rooms r(workspace);
  const CensusRooms ws(r, nx, ny);
  if (hipError_t e = census_clear(ws, workspace, stream)) {
    return e;
  }
  return census_score(p, (long long)nparticles, nx, ny, ws, NoGroups{}, UnitCells{}, stream);
}

size_t census_groups_workspace_bytes(int nx, int ny, int ngroups) {
  return bytes_of<GroupCensusRooms>(nx, ny, ngroups);
}

hipError_t launch_census_score_groups(const ParticleView& p, int nparticles, int nx, int ny, int ngroups,
                                      const double* host_edges, void* workspace, hipStream_t stream) {
  if (ngroups < 1 || ngroups > kSpectrumMaxGroups) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const GroupCensusRooms ws(r, nx, ny, ngroups);
  if (hipError_t e = census_clear(ws, workspace, stream)) {
    return e;
  }
  /* (host_edges stays the caller's until the stream has drained) */
  if (hipError_t e = hipMemcpyAsync(ws.edges, host_edges, sizeof(double) * (size_t)(ngroups + 1),
                                    hipMemcpyHostToDevice, stream)) {
    return e;
  }
  return census_score(p, (long long)nparticles, nx, ny, ws,
                      EnergyGroups{ws.edges, ngroups, &ws.header->groups.outside}, UnitCells{}, stream);
}

namespace {
BlockCells block_cells(const BlockMesh& b) {
  return BlockCells{b.cnx, b.cny, BlockDivisor::of(b.block_x), BlockDivisor::of(b.block_y)};
}
}  // namespace

hipError_t launch_census_score_blocks(const ParticleView& p, int nparticles, int nx, int ny, const BlockMesh& b,
                                      int ngroups, const double* host_edges, int lds_max_bins,
                                      int compute_units, void* workspace, hipStream_t stream,
                                      bool* privatised) {
  if (ngroups < 0 || ngroups > kSpectrumMaxGroups) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const GroupCensusRooms ws(r, b.cnx, b.cny, ngroups > 0 ? ngroups : 1);
  if (hipError_t e = census_clear(ws, workspace, stream)) {
    return e;
  }
  const int cap = lds_max_bins < kCensusLdsBinsMax ? lds_max_bins : kCensusLdsBinsMax;
  const CensusLds lds{nparticles > 0 && (long long)ws.cells <= (long long)cap, compute_units};
  *privatised = lds.on;
  if (ngroups == 0) {
    return census_score(p, (long long)nparticles, nx, ny, ws, NoGroups{}, block_cells(b), stream, lds);
  }
  /* (host_edges stays the caller's until the stream has drained) */
  if (hipError_t e = hipMemcpyAsync(ws.edges, host_edges, sizeof(double) * (size_t)(ngroups + 1),
                                    hipMemcpyHostToDevice, stream)) {
    return e;
  }
  return census_score(p, (long long)nparticles, nx, ny, ws,
                      EnergyGroups{ws.edges, ngroups, &ws.header->groups.outside}, block_cells(b), stream, lds);
}

hipError_t launch_census_finish(int nx, int ny, double* out, void* workspace, hipStream_t stream) {
  Rooms r(workspace);
  const CensusRooms ws(r, nx, ny);
  CensusHeader* header = &ws.header->census;
  const double* mesh = ws.mesh;
  const long long cells = (long long)ws.cells;
  const double* occupied = reduce<SumF64>(CensusOccupiedIn{mesh, cells}, cells, ws.sums[0], stream);
  const double* max_count = reduce<MaxF64>(CensusCountIn{mesh, cells}, cells, ws.sums[1], stream);
  const double* weight = reduce<SumF64>(CensusWeightIn{mesh, cells}, cells, ws.sums[2], stream);
  const double* max_weight = reduce<MaxF64>(CensusWeightIn{mesh, cells}, cells, ws.sums[3], stream);
  hipLaunchKernelGGL(census_decide_kernel, dim3(1), dim3(1), 0, stream, header, mesh + 2 * cells, occupied,
                     max_count, weight, max_weight);
  hipLaunchKernelGGL(census_fill_kernel, dim3((unsigned)((cells + kCombBlock - 1) / kCombBlock)),
                     dim3(kCombBlock), 0, stream, (const CensusHeader*)header, mesh, out, cells);
  return hipGetLastError();
}

hipError_t launch_bounds(const BoundsArgs& a, double* lower_out, void* workspace, hipStream_t stream) {
  Rooms r(workspace);
  const CensusRooms ws(r, a.nx, a.ny);
  BoundsHeader* header = &ws.header->bounds;
  const long long cells = (long long)ws.cells;
  const double* eligible = reduce<SumF64>(BoundsEligibleIn{a}, cells, ws.sums[0], stream);
  const double* max_weight = reduce<MaxF64>(BoundsWeightIn{a}, cells, ws.sums[1], stream);
  const double* bad = reduce<MaxF64>(BoundsBadIn{a.census, cells}, cells, ws.sums[2], stream);
  hipLaunchKernelGGL(bounds_decide_kernel, dim3(1), dim3(1), 0, stream, header, a, eligible, max_weight, bad);
  hipLaunchKernelGGL(bounds_fill_kernel, dim3((unsigned)((cells + kCombBlock - 1) / kCombBlock)),
                     dim3(kCombBlock), 0, stream, header, a, lower_out);
  return hipGetLastError();
}

size_t comb_workspace_bytes(int n) { return bytes_of<CombRooms>((long long)n); }
size_t window_workspace_bytes(int n) { return bytes_of<WindowRooms>((long long)n); }

hipError_t launch_comb(const ParticleView& p, int nparticles, uint64_t pkey, uint64_t seed,
                       void* workspace, hipStream_t stream) {
  const long long n = nparticles;
  Rooms r(workspace);
  const CombRooms ws(r, n);
  CombHeader* header = ws.header;
  unsigned* teeth = ws.teeth;
  unsigned* src = ws.src;

  hipLaunchKernelGGL(comb_begin_kernel, dim3(1), dim3(1), 0, stream, header, pkey, seed);

  /* the weight scan into the tooth counts, and their running maximum */
  TeethOut teeth_out;
  teeth_out.weight = p.weight;
  teeth_out.dead = p.dead;
  teeth_out.teeth = teeth;
  teeth_out.header = header;
  teeth_out.n = n;
  if (hipError_t e = scan<SumF64>(LiveWeightIn{p.weight, p.dead}, n, ws.sums, teeth_out, stream)) {
    return e;
  }
  if (hipError_t e = scan_in_place<MaxU32>(teeth, n, (unsigned*)ws.sums, stream)) {
    return e;
  }
  hipLaunchKernelGGL(comb_decide_kernel, dim3(1), dim3(1), 0, stream, header, n);

  /* src[]: heads, then the running maximum */
  const unsigned blocks = (unsigned)((n + kCombBlock - 1) / kCombBlock);
  hipLaunchKernelGGL(comb_clear_kernel, dim3(blocks), dim3(kCombBlock), 0, stream, header, src, n);
  hipLaunchKernelGGL(comb_heads_kernel, dim3(blocks < 4096u ? blocks : 4096u), dim3(kCombBlock), 0,
                     stream, header, teeth, src, n);
  if (hipError_t e = scan_in_place<MaxU32>(src, n, (unsigned*)ws.sums, stream)) {
    return e;
  }

  /* the gather, field by field through the scratch */
  double* const f64_fields[] = {p.x, p.y, p.omega_x, p.omega_y, p.energy, p.dt_to_census,
                                p.mfp_to_collision};
  for (double* field : f64_fields) {
    hipLaunchKernelGGL(comb_gather_kernel<double>, dim3(blocks), dim3(kCombBlock), 0, stream, header,
                       field, src, ws.scratch, n);
    hipLaunchKernelGGL(comb_copy_back_kernel<double>, dim3(blocks), dim3(kCombBlock), 0, stream,
                       header, ws.scratch, field, n);
  }
  hipLaunchKernelGGL(comb_gather_cells_kernel, dim3(blocks), dim3(kCombBlock), 0, stream, header,
                     p.cellx, p.celly, src, (int2*)ws.scratch, n);
  hipLaunchKernelGGL(comb_finish_kernel, dim3(blocks), dim3(kCombBlock), 0, stream, header,
                     (const int2*)ws.scratch, p.cellx, p.celly, p.weight, p.dead, n);
  return hipGetLastError();
}

/* What the three sources begin with: the header cleared where it has more than the base (which the
 * scan's last lane fills), and the scan of the dead flags into the list.  *most: the lanes a fill
 * can need, min(count, n). */
namespace {

SourceHeader* base_of(SourceHeader* h) { return h; }
template <class Header>
SourceHeader* base_of(Header* h) {
  return &h->base;
}
template <class Header>
hipError_t list_dead_slots(const SourceRooms<Header>& ws, const InjectArgs& a, long long n, int count,
                           unsigned* most, hipStream_t stream) {
  *most = (unsigned)((long long)count < n ? (long long)count : n);
  if (sizeof(Header) > sizeof(SourceHeader)) {
    if (hipError_t e = hipMemsetAsync(ws.header, 0, sizeof(Header), stream)) {
      return e;
    }
  }
  return scan<SumU32>(DeadIn{a.p.dead}, n, ws.sums,
                      SourceListOut{a.p.dead, ws.list, base_of(ws.header), n, (unsigned)count}, stream);
}

}  // namespace

size_t source_workspace_bytes(int n) { return bytes_of<SourceRooms<SourceHeader>>((long long)n); }

hipError_t launch_source(const InjectArgs& a, int nparticles, int count, double weight, uint64_t seed,
                         void* workspace, hipStream_t stream) {
  const long long n = nparticles;
  Rooms r(workspace);
  const SourceRooms<SourceHeader> ws(r, n);
  unsigned most;
  if (hipError_t e = list_dead_slots(ws, a, n, count, &most, stream)) {
    return e;
  }
  if (most > 0) {
    hipLaunchKernelGGL(source_fill_kernel, dim3((most + kCombBlock - 1) / kCombBlock), dim3(kCombBlock),
                       0, stream, a, (const SourceHeader*)ws.header, (const unsigned*)ws.list, seed, weight);
  }
  return hipGetLastError();
}

size_t described_workspace_bytes(int n) { return bytes_of<DescribedRooms>((long long)n); }

hipError_t launch_described_source(const InjectArgs& a, int nparticles, int count, double weight,
                                   uint64_t seed, const DescribedTables* host_tables, int ncomponents,
                                   int nbins, void* workspace, hipStream_t stream) {
  const long long n = nparticles;
  if (ncomponents < 1 || ncomponents > kDescribedMaxComponents || nbins < 1 || nbins > kDescribedMaxBins) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const DescribedRooms ws(r, n);
  unsigned most;
  if (hipError_t e = list_dead_slots(ws, a, n, count, &most, stream)) {
    return e;
  }
  if (most > 0) {
    /* (host_tables stays the caller's until the stream has drained) */
    if (hipError_t e = hipMemcpyAsync(ws.tables, host_tables, sizeof(DescribedTables),
                                      hipMemcpyHostToDevice, stream)) {
      return e;
    }
    const unsigned blocks = (most + kCombBlock - 1) / kCombBlock;
    hipLaunchKernelGGL(described_fill_kernel,
                       dim3(blocks < kDescribedFillBlocks ? blocks : kDescribedFillBlocks), dim3(kCombBlock),
                       0, stream, a, ws.header, (const unsigned*)ws.list, (const DescribedTables*)ws.tables,
                       ncomponents, nbins, seed, weight);
  }
  return hipGetLastError();
}

size_t mesh_source_workspace_bytes(int n, long long cells) {
  return bytes_of<MeshSourceRooms>((long long)n, cells);
}

hipError_t launch_mesh_source(const InjectArgs& a, int nparticles, int count, double weight, uint64_t seed,
                              const MeshSourceArgs& m, const MeshSourceBins* host_bins, void* workspace,
                              hipStream_t stream) {
  const long long n = nparticles;
  const long long cells = (long long)a.local_nx * a.local_ny;
  if (cells < 1 || cells > kMeshSourceMaxCells || m.nbins < 1 || m.nbins > kDescribedMaxBins) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const MeshSourceRooms ws(r, n, cells);
  MeshSourceHeader* header = ws.header;
  unsigned most;
  if (hipError_t e = list_dead_slots(ws, a, n, count, &most, stream)) {
    return e;
  }
  /* the mesh: ranks, then the cumulative sums at them (a mesh the call refuses is refused whether
   * or not a slot is dead) */
  MeshRankOut rank_out;
  rank_out.strength = m.strength;
  rank_out.rank = ws.rank;
  rank_out.header = header;
  rank_out.cells = cells;
  if (hipError_t e = scan<SumU32>(StrengthPositiveIn{m.strength}, cells, (unsigned*)ws.mesh_sums, rank_out, stream)) {
    return e;
  }
  if (hipError_t e = scan<SumF64>(StrengthIn{m.strength}, cells, ws.mesh_sums,
                                  MeshCumulativeOut{m.strength, ws.rank, ws.cumulative, ws.cell_of, header, cells},
                                  stream)) {
    return e;
  }
  hipLaunchKernelGGL(mesh_source_decide_kernel, dim3(1), dim3(1), 0, stream, header);
  if (most > 0) {
    /* (host_bins stays the caller's until the stream has drained) */
    if (hipError_t e = hipMemcpyAsync(ws.bins, host_bins, sizeof(MeshSourceBins), hipMemcpyHostToDevice,
                                      stream)) {
      return e;
    }
    const unsigned blocks = (most + kCombBlock - 1) / kCombBlock;
    hipLaunchKernelGGL(mesh_fill_kernel<kMeshCoarse>, dim3(blocks < kMeshFillBlocks ? blocks : kMeshFillBlocks),
                       dim3(kCombBlock), 0, stream, a, (const MeshSourceHeader*)header, (const unsigned*)ws.list,
                       (const double*)ws.cumulative, (const unsigned*)ws.cell_of, (const MeshSourceBins*)ws.bins,
                       m, seed, weight);
  }
  return hipGetLastError();
}

size_t bank_source_workspace_bytes(int n) { return bytes_of<SourceRooms<BankSourceHeader>>((long long)n); }

hipError_t launch_bank_source(const InjectArgs& a, int nparticles, int count, const BankSourceArgs& b,
                              void* workspace, hipStream_t stream) {
  const long long n = nparticles;
  Rooms r(workspace);
  const SourceRooms<BankSourceHeader> ws(r, n);
  unsigned most;
  if (hipError_t e = list_dead_slots(ws, a, n, count, &most, stream)) {
    return e;
  }
  hipLaunchKernelGGL(bank_begin_kernel, dim3(1), dim3(1), 0, stream, ws.header);
  if (most > 0) {
    const dim3 grid((most + kCombBlock - 1) / kCombBlock);
    hipLaunchKernelGGL(bank_check_kernel, grid, dim3(kCombBlock), 0, stream, a, ws.header, b);
    hipLaunchKernelGGL(bank_fill_kernel, grid, dim3(kCombBlock), 0, stream, a, ws.header, (const unsigned*)ws.list, b);
  }
  return hipGetLastError();
}

namespace {

WindowHeader* window_of(WindowHeader* h) { return h; }
WindowHeader* window_of(GroupWindowHeader* h) { return &h->window; }

/* either window: the header is cleared whole, the two kernels that look a bound up know of the
 * groups, and everything between them sees the byte per slot and never a cell */
template <class Header, class Groups, class Cells>
hipError_t window_passes(const ParticleView& p, long long n, const WindowArgs& a,
                         const WindowRoomsOf<Header>& ws, Groups groups, Cells cells, hipStream_t stream) {
  WindowHeader* header = window_of(ws.header);
  double* new_weight = ws.new_weight;
  unsigned* list = ws.list;
  unsigned* owner = ws.owner;
  unsigned char* code = ws.code;

  const unsigned tiles = tiles_of(n);
  const unsigned blocks = (unsigned)((n + kCombBlock - 1) / kCombBlock);
  const unsigned strided = blocks < 4096u ? blocks : 4096u;

  hipLaunchKernelGGL(window_begin_kernel<Header>, dim3(1), dim3(1), 0, stream, ws.header);
  /* (the classification: a tile's worth of slots per workgroup at least, 2 048 workgroups at most) */
  hipLaunchKernelGGL((window_classify_kernel<Groups, Cells>), dim3(tiles < 2048u ? tiles : 2048u),
                     dim3(kCombBlock), 0, stream, p, a, code, header, n, groups, cells);

  /* the free slots in ascending order, and their number */
  if (hipError_t e = scan<SumU32>(WindowFreeIn{code}, n, (unsigned*)ws.sums,
                                  WindowListOut{code, list, header, n}, stream)) {
    return e;
  }
  hipLaunchKernelGGL(window_decide_kernel, dim3(1), dim3(1), 0, stream, header);

  /* owner[]: heads from the demand scan, then the running maximum */
  hipLaunchKernelGGL(window_clear_kernel, dim3(strided), dim3(kCombBlock), 0, stream,
                     (const WindowHeader*)header, owner);
  WindowHeadsOut heads;
  heads.code = code;
  heads.weight = p.weight;
  heads.owner = owner;
  heads.new_weight = new_weight;
  heads.header = header;
  if (hipError_t e = scan<SumU64>(WindowDemandIn{code}, n, ws.sums, heads, stream)) {
    return e;
  }
  if (hipError_t e = scan<MaxU32>(WindowOwnerIn{owner, header}, n, (unsigned*)ws.sums,
                                  WindowOwnerOut{owner, header}, stream)) {
    return e;
  }

  /* the stores: roulette's first, the copies after them */
  hipLaunchKernelGGL((window_roulette_kernel<Groups, Cells>), dim3(strided), dim3(kCombBlock), 0, stream, p, a,
                     (const unsigned char*)code, (const WindowHeader*)header, n, groups, cells);
  hipLaunchKernelGGL(window_fill_kernel, dim3(strided), dim3(kCombBlock), 0, stream, p,
                     (const WindowHeader*)header, (const unsigned*)owner, (const unsigned*)list,
                     (const double*)new_weight);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_window(const ParticleView& p, int nparticles, const WindowArgs& a, void* workspace,
                         hipStream_t stream) {
  Rooms r(workspace);
  const WindowRooms ws(r, (long long)nparticles);
  return window_passes(p, (long long)nparticles, a, ws, NoGroups{}, UnitCells{}, stream);
}

size_t window_groups_workspace_bytes(int n) { return bytes_of<GroupWindowRooms>((long long)n); }

hipError_t launch_window_groups(const ParticleView& p, int nparticles, const WindowArgs& a, int ngroups,
                                const double* host_edges, void* workspace, hipStream_t stream) {
  if (ngroups < 1 || ngroups > kSpectrumMaxGroups) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const GroupWindowRooms ws(r, (long long)nparticles);
  /* (host_edges stays the caller's until the stream has drained) */
  if (hipError_t e = hipMemcpyAsync(ws.edges, host_edges, sizeof(double) * (size_t)(ngroups + 1),
                                    hipMemcpyHostToDevice, stream)) {
    return e;
  }
  return window_passes<GroupWindowHeader>(p, (long long)nparticles, a, ws,
                                          EnergyGroups{ws.edges, ngroups, &ws.header->outside}, UnitCells{},
                                          stream);
}

hipError_t launch_window_blocks(const ParticleView& p, int nparticles, const WindowArgs& a, const BlockMesh& b,
                                int ngroups, const double* host_edges, void* workspace, hipStream_t stream) {
  if (ngroups < 0 || ngroups > kSpectrumMaxGroups) {
    return hipErrorInvalidValue;
  }
  Rooms r(workspace);
  const GroupWindowRooms ws(r, (long long)nparticles);
  if (ngroups == 0) { /* (the grouped header, its counter left at 0) */
    return window_passes<GroupWindowHeader>(p, (long long)nparticles, a, ws, NoGroups{}, block_cells(b), stream);
  }
  if (hipError_t e = hipMemcpyAsync(ws.edges, host_edges, sizeof(double) * (size_t)(ngroups + 1),
                                    hipMemcpyHostToDevice, stream)) {
    return e;
  }
  return window_passes<GroupWindowHeader>(p, (long long)nparticles, a, ws,
                                          EnergyGroups{ws.edges, ngroups, &ws.header->outside}, block_cells(b),
                                          stream);
}

}  // namespace neutral
