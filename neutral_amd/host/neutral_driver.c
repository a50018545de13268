/*
 * neutral_driver.c -- `neutral.hip`: stand-alone driver of the MI355X kernel
 * set, for machines where the reference tree is not at hand.  It drives the
 * three interface functions (neutral_interface.h:11-36) the way the reference's
 * main.c + neutral_data.c do -- deck, mesh, density, source box, injection,
 * cross-section tables, timestep loop, validation -- and prints the same
 * per-step lines (main.c:88,118-125,161-162), so logs are comparable line by
 * line.  Everything numerical happens behind the C ABI (include/neutral_hip.h).
 *
 *   neutral.hip <deck.params> [--set key=value ...] [--arch-params FILE]
 *               [--cs-dir DIR] [--tests FILE] [--variant 0|1|2] [--gpus N]
 *               [--decompose PXxPY] [--current] [--outflow] [--vacuum SIDES] [--periodic AXES] [--comb EVERY]
 *               [--leakage M[,E0,...,EG]] [--escape-bank CAPACITY[,PATH]] [--source-bank PATH[,SNAP]]
 *               [--source COUNT[,WEIGHT]] [--source-file PATH | --source-mesh PATH]
 *               [--window WLOW|auto[,UPPER_RATIO[,SURVIVAL_RATIO]]]
 *               [--window-in-step]
 *               [--window-groups E0,E1,...,EG] [--window-block BX[,BY]] [--batches B]
 *
 * --gpus N runs N ranks, one per GPU of this node: the driver forks them before
 * anything touches a GPU (ranks are ordinary processes that find each other through
 * RANK / WORLD_SIZE / MASTER_PORT, so any launcher that exports those -- torchrun
 * --no-python, for one -- does as well); particles are sharded, every rank holds
 * the mesh, and each timestep ends with one all-reduce of the tally (RCCL).
 * --decompose PXxPY (PX * PY = N) cuts the MESH over the ranks instead: every rank
 * holds one block of it and the particles inside; histories that cross between
 * blocks are exchanged within the timestep (include/neutral_hip.h).
 *
 * --comb EVERY runs the census weight comb (include/neutral_hip.h) after every EVERY-th
 * timestep, seeded with the timestep's number: every slot alive again at one weight.  Not with
 * --decompose.
 *
 * --source COUNT[,WEIGHT] runs the fixed source (include/neutral_hip.h) before every timestep
 * tt >= 2, seeded with 2^63 + tt: up to COUNT dead slots become new source particles of WEIGHT
 * (default 1).  Several ranks emit their shares of COUNT, split as injection splits the particles.
 * Not with --decompose.
 * --source-file PATH, together with --source, makes those particles out of a described source
 * (include/neutral_hip.h: neutral_hip_source_described) instead of the deck's: a file in the decks'
 * key=value style, in which
 *   component share= xpos= ypos= width= height= [theta0= theta_width=]
 * opens a component (every direction unless it says otherwise) and
 *   line energy= share=          bin lo= hi= share=
 * add a line or a bin of its spectrum to the last component opened.  One `Source component K
 * emitted M` line per component joins the totals.  The initial population stays the deck's.
 * --source-mesh PATH, together with --source and instead of --source-file, makes those particles
 * out of a mesh source (include/neutral_hip.h: neutral_hip_source_mesh): a text file whose first
 * line is `nx ny`, the deck's mesh, followed by nx * ny strengths in row order (`#` starts a
 * comment); a particle is born in a cell in proportion to its strength, in every direction, at the
 * deck's initial energy.  One `Source mesh emitted M from K cells` line joins the totals.
 *
 * --window WLOW[,UPPER_RATIO[,SURVIVAL_RATIO]] applies the census weight window
 * (include/neutral_hip.h) after every timestep but the last, seeded with 2^63 + 2^62 + tt: the
 * lower bound WLOW in every cell, histories over UPPER_RATIO * WLOW (default 5) split into at most
 * 5, histories under WLOW playing roulette for SURVIVAL_RATIO * WLOW (default 3).  Several ranks
 * window their own shards.  Not with --decompose.
 * --window auto[,UPPER_RATIO[,SURVIVAL_RATIO]] makes the bounds itself, at the same point: the
 * census tally of the store (one `Census ...` line per call), bounds proportional to the cells'
 * weight for as many histories as are alive (neutral_hip_window_bounds, floor_ratio 0, min_count
 * 1), then the window with them.  A census or bounds that finds nothing usable -- an empty store --
 * skips that step's window and is counted (`Window auto skipped`).
 * --window-in-step, only together with --window, also puts the mesh of lower bounds that --window
 * applies at the census -- uniform, or auto's latest bounds (none before the first census) -- in force
 * DURING the steps (include/neutral_hip.h: neutral_hip_set_window_roulette): an absorption that leaves
 * a weight under its bin's bound plays roulette for SURVIVAL_RATIO times the bound.  With
 * --window-groups and --window-block the bins are theirs.  Works with --gpus N, and --window WLOW
 * --window-in-step with --decompose too, where the census window itself does not run.  Not with
 * --roulette.  Prints the `Roulette killed` / `Roulette survived` lines as --roulette does.
 * --window-groups E0,E1,...,EG, only together with --window, keys both forms on (cell, energy group)
 * bins (include/neutral_hip.h: energy groups for the census tally and the weight window): 1 to 64
 * groups with finite, positive, strictly ascending edges.  --window WLOW then gives every bin the
 * bound WLOW; --window auto runs the grouped census, the bounds over the bins (for as many
 * histories as are alive inside the groups) and the grouped window.  A live history in no group has
 * no window; one `Window outside N` line joins the totals: such histories met, summed over the
 * windows (with auto: over their censuses, so that a step whose window is skipped counts too).
 * --window-block BX[,BY] (BY defaults to BX), only together with --window, keys both forms on blocks
 * of BX by BY cells (include/neutral_hip.h: a coarse window mesh), with or without --window-groups:
 * on a sparse deck, where a cell holds one history or none, that is the mesh a window has something
 * to work on.  --window WLOW gives every bin the bound WLOW; --window auto runs the blocks census,
 * the bounds over the bins and the blocks window.  One `Window blocks CNX x CNY` line joins the
 * totals.  Not with --decompose.
 *
 * --batches B runs the deck's N particles as B independent batches of N / B, one after the other
 * through all the timesteps, each with its own particle ids (include/neutral_hip.h: batch
 * statistics): the energy deposition of every batch is folded into running moments on the device
 * (neutral_hip_batch_fold), and what is validated and summed at the end is the estimate of all the
 * batches together (neutral_hip_batch_statistics), printed with its standard error, the relative
 * error over the scored cells and the figure of merit 1 / (mean relerr^2 * wall seconds).  --comb,
 * --source, --window and the optional tallies keep their meaning inside each batch; the optional
 * tallies add up over the batches.  B >= 2 divides N.  Not with --gpus N > 1 or --decompose.
 *
 * --vacuum SIDES (letters of wesn, or all) makes those outer sides of the mesh vacuum
 * (include/neutral_hip.h: neutral_hip_set_vacuum_sides): a history that would reflect there escapes,
 * and every step prints `Escaped  west N (W) east N (W) south N (W) north N (W)` behind its
 * `Particles` line -- the histories that left through each side and the weight they took along.
 * With --outflow the entries of the outflow's meshes on those sides are the leakage per facet.
 * Works with every other option.
 * --periodic AXES (x, y or xy) makes the outer sides of those axes one seam (include/neutral_hip.h:
 * neutral_hip_set_periodic_axes): a history that would reflect there goes on from the opposite side
 * in the same step, and every step prints `Wrapped  west N (W) east N (W) south N (W) north N (W)`
 * behind its `Particles` line -- the histories that wrapped by the side they left through and the
 * weight they carried.  Not with --vacuum on a side of the same axis.
 * --leakage M[,E0,E1,...,EG], only together with --vacuum, keeps the leakage tally (include/neutral_hip.h:
 * neutral_hip_set_leakage_tally): the escapes by side, by energy group -- 0 to 64 groups with finite,
 * positive, strictly ascending edges -- and by M = 1 to 64 bins of the cosine between the direction
 * and the outward normal.  At the end of the run one block per vacuum side: a `Leakage SIDE group K
 * [E_K, E_K+1)` line per group and a `Leakage SIDE no group` line, each with the weight over N per
 * cosine bin, then `Leakage SIDE total COUNT (WEIGHT)`, the sums of the side's `Escaped` figures.
 *
 * --escape-bank CAPACITY[,PATH], only together with --vacuum, keeps the escape bank (include/neutral_hip.h:
 * neutral_hip_set_escape_bank): every history that leaves, 64 bytes each, up to CAPACITY of them.  Every step
 * prints `Banked: CLAIMED RECORDED`, the bank's cursor and what it holds, behind its `Escaped` line; at the
 * end PATH is written: the 8 bytes NHBANK01, a u64 count, then the records in bank order.  With more than
 * one rank every rank keeps its own bank and writes PATH.<rank>.
 * --source-bank PATH[,SNAP], together with --source COUNT and instead of --source-file / --source-mesh,
 * emits up to COUNT records of such a file before every timestep from the second, continuing where the
 * last emission stopped (include/neutral_hip.h: neutral_hip_source_bank; SNAP: the snap distance, 0 without
 * it; no shift, weights as recorded -- --source's WEIGHT scales them).  With more than one rank every rank
 * reads PATH.<rank>.  Neither works with --decompose.
 *
 * --set overrides a scalar deck entry (nx, ny, nparticles, iterations, dt,
 * initial_energy): the BASELINE configurations are the shipped decks at other
 * sizes.  ../arch.params (neutral_data.h:32) supplies width/height/sim_end when
 * present; otherwise 1.0 x 1.0, the extent the reference's known answers need.
 */
#include <arpa/inet.h>
#include <ctype.h>
#include <math.h>
#include <netinet/in.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "../../include/neutral_hip.h"
#include "comms.h"
#include "mesh.h"
#include "neutral_problem.h"
#include "params.h"
#include "shared.h"
#include "shared_data.h"

#define MAX_OVERRIDES 16

static double now_seconds(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1.0e-9 * (double)ts.tv_nsec;
}

/* Writes a copy of `deck` with the scalar entries named in keys[] replaced. */
static void write_patched_deck(const char* deck, const char* out, int n, char keys[][64],
                               char values[][64]) {
  FILE* in = fopen(deck, "r");
  if (!in) {
    TERMINATE("Could not open the parameter file: %s.\n", deck);
  }
  FILE* fp = fopen(out, "w");
  if (!fp) {
    TERMINATE("Could not write %s.\n", out);
  }
  char line[4096];
  int used[MAX_OVERRIDES] = {0};
  while (fgets(line, sizeof(line), in)) {
    char first[256] = "";
    sscanf(line, " %255s", first);
    int replaced = 0;
    for (int k = 0; k < n; ++k) {
      if (strcmp(first, keys[k]) == 0) {
        fprintf(fp, "%s %s\n", keys[k], values[k]);
        used[k] = 1;
        replaced = 1;
      }
    }
    if (!replaced) {
      fputs(line, fp);
    }
  }
  for (int k = 0; k < n; ++k) {
    if (!used[k]) {
      fprintf(fp, "%s %s\n", keys[k], values[k]);
    }
  }
  fclose(in);
  fclose(fp);
}

/* One `key=value` token of a --source-file line into the slot of its key; -> 0 where the key is none
 * of keys[] or the value is not a number. */
static int source_file_value(const char* token, int nkeys, const char* const* keys, double* values,
                             int* seen) {
  const char* eq = strchr(token, '=');
  if (!eq) {
    return 0;
  }
  for (int k = 0; k < nkeys; ++k) {
    if (strlen(keys[k]) == (size_t)(eq - token) && strncmp(token, keys[k], (size_t)(eq - token)) == 0) {
      char* end = NULL;
      values[k] = strtod(eq + 1, &end);
      seen[k] = 1;
      return end != eq + 1 && *end == '\0';
    }
  }
  return 0;
}

/* --source-file: the description in `path` into the two tables of neutral_hip_source_described */
static void read_source_file(const char* path, NeutralHipSourceComponent* components, int* ncomponents,
                             NeutralHipSourceBin* bins, int* nbins) {
  static const char* const component_keys[7] = {"share", "xpos", "ypos", "width", "height", "theta0",
                                                "theta_width"};
  static const char* const line_keys[2] = {"energy", "share"};
  static const char* const bin_keys[3] = {"lo", "hi", "share"};
  FILE* fp = fopen(path, "r");
  if (!fp) {
    TERMINATE("Could not open the source file: %s.\n", path);
  }
  *ncomponents = *nbins = 0;
  char text[4096];
  int lineno = 0;
  while (fgets(text, sizeof(text), fp)) {
    ++lineno;
    char* hash = strchr(text, '#');
    if (hash) {
      *hash = '\0';
    }
    char* save = NULL;
    const char* kind = strtok_r(text, " \t\r\n", &save);
    if (!kind) {
      continue;
    }
    const int is_component = strcmp(kind, "component") == 0;
    const int is_line = strcmp(kind, "line") == 0;
    if (!is_component && !is_line && strcmp(kind, "bin") != 0) {
      TERMINATE("--source-file %s:%d: a line opens with component, line or bin, not %s\n", path, lineno, kind);
    }
    const char* const* keys = is_component ? component_keys : is_line ? line_keys : bin_keys;
    const int nkeys = is_component ? 7 : is_line ? 2 : 3;
    const int needed = is_component ? 5 : nkeys; /* (theta0 and theta_width may be left out) */
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0 * M_PI};
    int seen[7] = {0, 0, 0, 0, 0, 0, 0};
    for (const char* token = strtok_r(NULL, " \t\r\n", &save); token; token = strtok_r(NULL, " \t\r\n", &save)) {
      if (!source_file_value(token, nkeys, keys, v, seen)) {
        TERMINATE("--source-file %s:%d: bad number or unknown key in %s\n", path, lineno, token);
      }
    }
    for (int k = 0; k < needed; ++k) {
      if (!seen[k]) {
        TERMINATE("--source-file %s:%d: %s wants %s=\n", path, lineno, kind, keys[k]);
      }
    }
    if (is_component) {
      if (*ncomponents == 16) {
        TERMINATE("--source-file %s:%d: more than 16 components\n", path, lineno);
      }
      const NeutralHipSourceComponent c = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], *nbins, 0};
      components[(*ncomponents)++] = c;
    } else {
      if (*ncomponents == 0) {
        TERMINATE("--source-file %s:%d: a %s before any component\n", path, lineno, kind);
      }
      if (*nbins == 256) {
        TERMINATE("--source-file %s:%d: more than 256 lines and bins\n", path, lineno);
      }
      const NeutralHipSourceBin b = {v[0], is_line ? v[0] : v[1], is_line ? v[1] : v[2]};
      bins[(*nbins)++] = b;
      components[*ncomponents - 1].bin_count++;
    }
  }
  fclose(fp);
  if (*ncomponents == 0) {
    TERMINATE("--source-file %s: no component\n", path);
  }
  for (int k = 0; k < *ncomponents; ++k) {
    if (components[k].bin_count == 0) {
      TERMINATE("--source-file %s: component %d has no line or bin\n", path, k);
    }
  }
}

/* The next token of a --source-mesh file into buf: characters up to white space, whatever the length
 * of the line; `#` starts a comment that runs to the end of its line.  -> 1, or 0 at the end of the
 * file; *lineno is the line the token stands on.  A token of `cap` characters or more is handed
 * back cut: no number is that long, and strtol / strtod refuse what is left of it. */
static int source_mesh_token(FILE* fp, char* buf, size_t cap, int* lineno) {
  int c = fgetc(fp);
  for (;;) {
    if (c == '#') {
      while (c != EOF && c != '\n') {
        c = fgetc(fp);
      }
    }
    if (c == EOF) {
      return 0;
    }
    if (c != ' ' && c != '\t' && c != '\r' && c != '\n') {
      break;
    }
    if (c == '\n') {
      ++*lineno;
    }
    c = fgetc(fp);
  }
  size_t len = 0;
  while (c != EOF && c != ' ' && c != '\t' && c != '\r' && c != '\n' && c != '#') {
    if (len + 1 < cap) {
      buf[len++] = (char)c;
    } else {
      buf[0] = '?'; /* (too long to be a number) */
    }
    c = fgetc(fp);
  }
  if (c != EOF) {
    ungetc(c, fp);
  }
  buf[len] = '\0';
  return 1;
}

/* --source-mesh: the strengths in `path`, nx * ny of them behind the line `nx ny`, which must be the
 * deck's mesh (checked before anything is allocated); -> a host array of the caller's
 * (allocate_host_data) */
static double* read_source_mesh_file(const char* path, int nx, int ny) {
  FILE* fp = fopen(path, "r");
  if (!fp) {
    TERMINATE("Could not open the source mesh: %s.\n", path);
  }
  char token[64];
  int lineno = 1;
  long sizes[2] = {0, 0};
  for (int k = 0; k < 2; ++k) {
    char* end = NULL;
    if (!source_mesh_token(fp, token, sizeof(token), &lineno)) {
      TERMINATE("--source-mesh %s: too few numbers: `nx ny` and nx * ny strengths\n", path);
    }
    sizes[k] = strtol(token, &end, 10);
    if (end == token || *end != '\0' || sizes[k] < 1 || sizes[k] > 2147483647L) {
      TERMINATE("--source-mesh %s:%d: the first line is `nx ny`, not %s\n", path, lineno, token);
    }
  }
  if (sizes[0] != nx || sizes[1] != ny) {
    TERMINATE("--source-mesh %s holds %ld x %ld cells: the deck's mesh is %d x %d\n", path, sizes[0], sizes[1],
              nx, ny);
  }
  const size_t cells = (size_t)nx * (size_t)ny;
  double* strength = NULL;
  allocate_host_data(&strength, cells);
  size_t have = 0;
  while (source_mesh_token(fp, token, sizeof(token), &lineno)) {
    char* end = NULL;
    const double v = strtod(token, &end);
    if (end == token || *end != '\0') {
      TERMINATE("--source-mesh %s:%d: bad number %s\n", path, lineno, token);
    }
    if (have == cells) {
      TERMINATE("--source-mesh %s:%d: more than %d x %d numbers\n", path, lineno, nx, ny);
    }
    strength[have++] = v;
  }
  fclose(fp);
  if (have < cells) {
    TERMINATE("--source-mesh %s: too few numbers: `nx ny` and nx * ny strengths\n", path);
  }
  return strength;
}

/* a TCP port nobody listens on right now (for the ranks' rendezvous) */
static int free_port(void) {
  const int fd = socket(AF_INET, SOCK_STREAM, 0);
  struct sockaddr_in sa;
  memset(&sa, 0, sizeof(sa));
  sa.sin_family = AF_INET;
  sa.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  socklen_t len = sizeof(sa);
  int port = 29611;
  if (fd >= 0 && bind(fd, (struct sockaddr*)&sa, sizeof(sa)) == 0 &&
      getsockname(fd, (struct sockaddr*)&sa, &len) == 0) {
    port = ntohs(sa.sin_port);
  }
  if (fd >= 0) close(fd);
  return port;
}

/* --gpus N: becomes rank 0..N-1 in N child processes (returns in the children with
 * the rank's environment set); the parent waits for them and exits with the worst
 * status.  Called before anything initialises a GPU. */
static void fork_ranks(int nranks) {
  char buf[32];
  snprintf(buf, sizeof(buf), "%d", free_port());
  setenv("MASTER_ADDR", "127.0.0.1", 1);
  setenv("MASTER_PORT", buf, 1);
  /* (the port that was just found free is the one the ranks meet on: left to its default --
   * MASTER_PORT + 1, comms_ranks.c -- the rendezvous would listen on a port nobody has looked at) */
  setenv("NEUTRAL_COMM_PORT", buf, 1);
  snprintf(buf, sizeof(buf), "%d", nranks);
  setenv("WORLD_SIZE", buf, 1);
  if (!getenv("NEUTRAL_COMM_NONCE")) {
    /* the word the ranks of THIS launch greet rank 0 with (comms_ranks.c) */
    unsigned long long nonce = ((unsigned long long)getpid() << 32) ^ (unsigned long long)time(NULL);
    FILE* rnd = fopen("/dev/urandom", "rb");
    if (rnd) {
      if (fread(&nonce, sizeof(nonce), 1, rnd) != 1) { /* keep the fallback */ }
      fclose(rnd);
    }
    snprintf(buf, sizeof(buf), "%llu", nonce);
    setenv("NEUTRAL_COMM_NONCE", buf, 1);
  }
  pid_t kids[64];
  for (int r = 0; r < nranks; ++r) {
    fflush(stdout);
    const pid_t pid = fork();
    if (pid < 0) {
      TERMINATE("Could not start rank %d.\n", r);
    }
    if (pid == 0) {
      snprintf(buf, sizeof(buf), "%d", r);
      setenv("RANK", buf, 1);
      setenv("LOCAL_RANK", buf, 1);
      return;
    }
    kids[r] = pid;
  }
  int worst = 0;
  for (int r = 0; r < nranks; ++r) {
    int status = 0;
    waitpid(kids[r], &status, 0);
    const int code = WIFEXITED(status) ? WEXITSTATUS(status) : 128 + WTERMSIG(status);
    worst = (code > worst) ? code : worst;
  }
  exit(worst);
}

/* the outer sides of the axes in a --periodic mask, as --vacuum numbers them (x: west and east; y: south and north) */
static unsigned sides_of_axes(unsigned axes) { return ((axes & 1u) ? 3u : 0u) | ((axes & 2u) ? 12u : 0u); }

static void load_table(const char* path, NeutralHipCrossSection* cs) {
  const int n = neutral_cs_file_entries(path);
  if (n < 0) {
    TERMINATE("Could not open the cross section file: %s\n", path);
  }
  if (comms_rank() == MASTER) {
    printf("File %s contains %d entries\n", path, n); /* neutral_data.c:139 */
  }
  double* h_keys;
  double* h_values;
  allocate_host_data(&h_keys, (size_t)n);
  allocate_host_data(&h_values, (size_t)n);
  cs->nentries = neutral_read_cs_file(path, n, h_keys, h_values);
  move_host_buffer_to_device((size_t)cs->nentries, &h_keys, &cs->keys);
  move_host_buffer_to_device((size_t)cs->nentries, &h_values, &cs->values);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    TERMINATE("usage: ./neutral.hip <param_file> [--set key=value ...] [--arch-params FILE] "
              "[--cs-dir DIR] [--tests FILE] [--variant N] [--collision-tallies] "
              "[--roulette WC,WS] [--spectrum E0,E1,...,EG[@X0,Y0,X1,Y1]] [--current] [--outflow] [--vacuum SIDES] [--periodic AXES] [--leakage M[,E0,...,EG]] [--escape-bank CAPACITY[,PATH]] [--source-bank PATH[,SNAP]] "
              "[--comb EVERY] [--source COUNT[,WEIGHT]] [--source-file PATH | --source-mesh PATH] "
              "[--window WLOW|auto[,UPPER_RATIO[,SURVIVAL_RATIO]]] [--window-in-step] [--window-groups E0,E1,...,EG] [--window-block BX[,BY]] "
              "[--batches B]\n");
  }
  const char* deck = argv[1];
  const char* arch_params = "../arch.params";
  const char* cs_dir = ".";
  char keys[MAX_OVERRIDES][64];
  char values[MAX_OVERRIDES][64];
  int noverrides = 0;
  int decompose_x = 0, decompose_y = 0;
  int collision_tallies = 0; /* --collision-tallies: keep them, print their totals at the end */
  int outflow = 0; /* --outflow: keep the outflow per side, print its sums and the wall hits at the end */
  unsigned periodic_axes = 0; /* --periodic AXES: histories wrap through the sides of those axes, a line per step */
  unsigned vacuum_sides = 0; /* --vacuum SIDES: histories escape through those outer sides, a line per step */
  /* --leakage M[,E0,...,EG]: the escapes by side, energy group and exit cosine, a block per vacuum side at the end */
  int leakage_cosines = 0, leakage_groups = 0;
  double leakage_edges[65];
  /* --escape-bank CAPACITY[,PATH]: the escaping histories themselves, a line per step, a file at the end */
  unsigned long long bank_capacity = 0;
  const char* bank_path = NULL;
  /* --source-bank PATH[,SNAP]: --source emits the records of such a file */
  char source_bank_path[4096] = "";
  double source_bank_snap = 0.0;
  int current = 0; /* --current: keep Jx, Jy (and the scalar flux), print their totals at the end */
  int roulette = 0; /* --roulette WC,WS: weight cutoff and survival weight, totals at the end */
  double roulette_cutoff = 0.0, roulette_survival = 0.0;
  unsigned long long roulette_killed = 0, roulette_survived = 0;
  /* --comb EVERY: the census weight comb after every EVERY-th timestep, totals at the end */
  int comb_every = 0;
  int combs = 0;
  unsigned long long comb_min_live = 0, comb_max_copies = 0;
  /* --source COUNT[,WEIGHT]: the fixed source before every timestep from the second, totals at the end */
  int source_count = 0;
  double source_weight = 1.0;
  unsigned long long source_emitted = 0;
  double source_weight_emitted = 0.0;
  /* --source-file PATH: ... out of a described source, per-component totals at the end */
  const char* source_file = NULL;
  NeutralHipSourceComponent source_components[16];
  NeutralHipSourceBin source_bins[256];
  int source_ncomponents = 0, source_nbins = 0;
  unsigned long long source_by_component[16] = {0};
  /* --source-mesh PATH: ... out of a mesh source, the cells it emits from at the end */
  const char* source_mesh_file = NULL;
  double* source_mesh_host = NULL;
  double* source_mesh = NULL; /* [device] the strengths */
  unsigned long long source_mesh_cells = 0;
  /* --window WLOW[,UPPER_RATIO[,SURVIVAL_RATIO]]: the census weight window after every timestep but
   * the last, totals at the end */
  int window = 0;
  double window_low = 0.0, window_upper = 5.0, window_survival = 3.0;
  const int window_max_split = 5;
  double* window_lower = NULL; /* [device] the uniform mesh of bounds, or what --window auto makes */
  int window_auto = 0;         /* --window auto: census, bounds, window */
  int window_in_step = 0;      /* --window-in-step: window_lower also plays inside the steps */
  double* window_census = NULL; /* [device] its census: counts, then weights */
  int window_skipped = 0;
  unsigned long long window_totals[5] = {0, 0, 0, 0, 0}; /* killed, survived, split, made, refused */
  /* --window-groups E0,...,EG: census, bounds and window over (cell, energy group) bins */
  int window_groups = 0;
  double window_edges[65];
  /* --window-block BX[,BY]: census, bounds and window over blocks of cells (0: the cells themselves) */
  int window_block_x = 0, window_block_y = 0;
  int window_cnx = 0, window_cny = 0; /* the mesh the bounds lie on: the deck's, or its blocks */
  unsigned long long window_outside = 0; /* live slots in no group, over the windows (auto: over the censuses) */
  /* --batches B: B independent batches of N / B particles, the statistics at the end */
  int batches = 0;
  double* batch_moments = NULL; /* [device] the energy tally's running means, then M2 */
  double* batch_relerr = NULL;  /* [device] its relative error per cell */
  /* --spectrum E0,...,EG[@X0,Y0,X1,Y1]: the flux spectrum over a box (default: the whole mesh),
   * one line per group at the end */
  int spectrum_groups = 0;
  double spectrum_edges[65];
  int spectrum_box[4] = {0, 0, -1, -1};
  /* multi-process GPU work on this stack needs dmabuf IPC; read by the runtime at start-up */
  setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0);
  int batches_asked = 0;
  for (int i = 2; i < argc; ++i) {
    batches_asked |= strcmp(argv[i], "--batches") == 0;
  }
  for (int i = 2; i + 1 < argc; ++i) {
    if (strcmp(argv[i], "--gpus") == 0) {
      const int n = atoi(argv[i + 1]);
      if (n < 1 || n > 64) {
        TERMINATE("--gpus wants 1..64\n");
      }
      if (n > 1 && batches_asked) {
        TERMINATE("--batches does not work with --gpus N > 1: a batch is not sharded over ranks\n");
      }
      if (n > 1 && !getenv("RANK")) {
        fork_ranks(n);
      }
    }
  }
  for (int i = 2; i < argc; ++i) {
    if (strcmp(argv[i], "--set") == 0 && i + 1 < argc && noverrides < MAX_OVERRIDES) {
      char* eq = strchr(argv[++i], '=');
      if (!eq) {
        TERMINATE("--set needs key=value\n");
      }
      snprintf(keys[noverrides], sizeof(keys[0]), "%.*s", (int)(eq - argv[i]), argv[i]);
      snprintf(values[noverrides], sizeof(values[0]), "%s", eq + 1);
      noverrides++;
    } else if (strcmp(argv[i], "--arch-params") == 0 && i + 1 < argc) {
      arch_params = argv[++i];
    } else if (strcmp(argv[i], "--cs-dir") == 0 && i + 1 < argc) {
      cs_dir = argv[++i];
    } else if (strcmp(argv[i], "--tests") == 0 && i + 1 < argc) {
      neutral_hip_set_tests_file(argv[++i]);
    } else if (strcmp(argv[i], "--gpus") == 0 && i + 1 < argc) {
      ++i; /* handled above, before anything touched a GPU */
    } else if (strcmp(argv[i], "--decompose") == 0 && i + 1 < argc) {
      if (sscanf(argv[++i], "%dx%d", &decompose_x, &decompose_y) != 2) {
        TERMINATE("--decompose wants PXxPY, e.g. 4x2\n");
      }
    } else if (strcmp(argv[i], "--collision-tallies") == 0) {
      collision_tallies = 1;
    } else if (strcmp(argv[i], "--current") == 0) {
      current = 1;
    } else if (strcmp(argv[i], "--outflow") == 0) {
      outflow = 1;
    } else if (strcmp(argv[i], "--vacuum") == 0) {
      const char* sides = (i + 1 < argc) ? argv[++i] : "";
      vacuum_sides = 0;
      if (strcmp(sides, "all") == 0) {
        vacuum_sides = 15;
      } else {
        for (const char* c = sides; *c; ++c) {
          const char* at = strchr("wesn", tolower((unsigned char)*c));
          if (!at) {
            vacuum_sides = 16; /* (refused below) */
            break;
          }
          vacuum_sides |= 1u << (unsigned)(at - "wesn");
        }
      }
      if (vacuum_sides < 16 && (vacuum_sides & sides_of_axes(periodic_axes))) {
        TERMINATE("--vacuum and --periodic name a side of the same axis: a wall wraps or leaks, not both\n");
      }
      if (vacuum_sides == 0 || neutral_hip_set_vacuum_sides(vacuum_sides) != 0) {
        TERMINATE("--vacuum wants SIDES: letters of wesn (west, east, south, north) or all, e.g. wn: histories "
                  "escape through those outer sides instead of reflecting\n");
      }
    } else if (strcmp(argv[i], "--periodic") == 0) {
      const char* axes = (i + 1 < argc) ? argv[++i] : "";
      periodic_axes = 0;
      for (const char* c = axes; *c; ++c) {
        const char* at = strchr("xy", tolower((unsigned char)*c));
        if (!at) {
          periodic_axes = 4; /* (refused below) */
          break;
        }
        periodic_axes |= 1u << (unsigned)(at - "xy");
      }
      if (periodic_axes < 4 && (vacuum_sides & sides_of_axes(periodic_axes))) {
        TERMINATE("--vacuum and --periodic name a side of the same axis: a wall wraps or leaks, not both\n");
      }
      if (periodic_axes == 0 || neutral_hip_set_periodic_axes(periodic_axes) != 0) {
        TERMINATE("--periodic wants AXES: x (west <-> east), y (south <-> north) or xy: histories wrap through "
                  "those outer sides instead of reflecting\n");
      }
    } else if (strcmp(argv[i], "--roulette") == 0 && i + 1 < argc) {
      if (sscanf(argv[++i], "%lf,%lf", &roulette_cutoff, &roulette_survival) != 2 ||
          neutral_hip_set_roulette(roulette_cutoff, roulette_survival) != 0) {
        TERMINATE("--roulette wants WC,WS with 0 <= WC <= WS, both 0 or neither, e.g. 0.25,0.5\n");
      }
      roulette = 1;
    } else if (strcmp(argv[i], "--comb") == 0) {
      char* end = NULL;
      const long every = (i + 1 < argc) ? strtol(argv[i + 1], &end, 10) : 0;
      if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || every < 1 || every > 1000000000) {
        TERMINATE("--comb wants EVERY >= 1: the comb runs after every EVERY-th timestep\n");
      }
      comb_every = (int)every;
      ++i;
    } else if (strcmp(argv[i], "--source") == 0) {
      char* end = NULL;
      const long count = (i + 1 < argc) ? strtol(argv[i + 1], &end, 10) : 0;
      int ok = i + 1 < argc && end != argv[i + 1] && count >= 1 && count <= 2147483647L;
      if (ok && *end == ',') {
        char* wend = NULL;
        source_weight = strtod(end + 1, &wend);
        ok = wend != end + 1 && *wend == '\0' && isfinite(source_weight) && source_weight > 0.0;
      } else if (ok) {
        ok = *end == '\0';
      }
      if (!ok) {
        TERMINATE("--source wants COUNT[,WEIGHT] with COUNT >= 1 and WEIGHT > 0: up to COUNT dead "
                  "slots are refilled before every timestep from the second\n");
      }
      source_count = (int)count;
      ++i;
    } else if (strcmp(argv[i], "--source-file") == 0) {
      if (i + 1 >= argc) {
        TERMINATE("--source-file wants PATH: the described source that --source emits from\n");
      }
      source_file = argv[++i];
    } else if (strcmp(argv[i], "--source-mesh") == 0) {
      if (i + 1 >= argc) {
        TERMINATE("--source-mesh wants PATH: the mesh of strengths that --source emits from\n");
      }
      source_mesh_file = argv[++i];
    } else if (strcmp(argv[i], "--escape-bank") == 0) {
      const char* spec = (i + 1 < argc) ? argv[++i] : "";
      char* end = NULL;
      bank_capacity = strtoull(spec, &end, 10);
      if (end == spec || spec[0] == '-' || bank_capacity < 1 || (*end != '\0' && *end != ',') ||
          (*end == ',' && end[1] == '\0')) {
        TERMINATE("--escape-bank wants CAPACITY[,PATH] with CAPACITY >= 1\n");
      }
      bank_path = (*end == ',') ? end + 1 : NULL;
    } else if (strcmp(argv[i], "--source-bank") == 0) {
      const char* spec = (i + 1 < argc) ? argv[++i] : "";
      const char* comma = strrchr(spec, ',');
      size_t len = strlen(spec);
      if (comma) {
        char* end = NULL;
        source_bank_snap = strtod(comma + 1, &end);
        if (end == comma + 1 || *end != '\0' || !isfinite(source_bank_snap) || source_bank_snap < 0.0) {
          TERMINATE("--source-bank wants PATH[,SNAP] with a finite SNAP >= 0\n");
        }
        len = (size_t)(comma - spec);
      }
      if (len == 0 || len >= sizeof(source_bank_path) - 16) {
        TERMINATE("--source-bank wants PATH[,SNAP]: the bank file that --source emits from\n");
      }
      memcpy(source_bank_path, spec, len);
      source_bank_path[len] = '\0';
    } else if (strcmp(argv[i], "--window") == 0) {
      /* one to three numbers, nothing after them */
      double v[3] = {0.0, window_upper, window_survival};
      int nv = 0;
      int ok = i + 1 < argc;
      const char* q = ok ? argv[i + 1] : "";
      int more = ok; /* numbers left to read */
      if (ok && strncmp(q, "auto", 4) == 0 && (q[4] == ',' || q[4] == '\0')) {
        window_auto = 1; /* (stands where WLOW would: the ratios, if any, follow) */
        v[0] = 1.0;
        nv = 1;
        more = q[4] == ',';
        q += 5;
      }
      while (more) {
        char* end = NULL;
        if (nv < 3) {
          v[nv] = strtod(q, &end);
        }
        ok = nv < 3 && end != q && isfinite(v[nv]) && (*end == ',' || *end == '\0');
        nv++;
        if (!ok || *end == '\0') {
          break;
        }
        q = end + 1;
      }
      ok = ok && nv >= 1 && v[0] > 0.0 && v[1] >= 2.0 && v[2] >= 1.0 && v[2] <= v[1];
      if (!ok && window_auto) {
        TERMINATE("--window wants auto[,UPPER_RATIO[,SURVIVAL_RATIO]] with UPPER_RATIO >= 2 and "
                  "1 <= SURVIVAL_RATIO <= UPPER_RATIO: census, bounds and window run after every "
                  "timestep but the last\n");
      }
      if (!ok) {
        TERMINATE("--window wants WLOW[,UPPER_RATIO[,SURVIVAL_RATIO]] with WLOW > 0, UPPER_RATIO >= 2 "
                  "and 1 <= SURVIVAL_RATIO <= UPPER_RATIO: the window runs after every timestep but "
                  "the last\n");
      }
      window = 1;
      window_low = v[0];
      window_upper = v[1];
      window_survival = v[2];
      ++i;
    } else if (strcmp(argv[i], "--window-in-step") == 0) {
      window_in_step = 1;
    } else if (strcmp(argv[i], "--window-groups") == 0) {
      /* two to 65 numbers, nothing after them: finite, positive, strictly ascending */
      int ok = i + 1 < argc;
      int nedges = 0;
      for (const char* q = ok ? argv[i + 1] : ""; ok;) {
        char* end = NULL;
        const double e = strtod(q, &end);
        ok = nedges < 65 && end != q && isfinite(e) && e > 0.0 && (nedges == 0 || e > window_edges[nedges - 1]) &&
             (*end == ',' || *end == '\0');
        if (!ok) {
          break;
        }
        window_edges[nedges++] = e;
        if (*end == '\0') {
          break;
        }
        q = end + 1;
      }
      if (!ok || nedges < 2) {
        TERMINATE("--window-groups wants E0,E1,...,EG with 1 to 64 groups, the edges finite, positive and "
                  "strictly ascending: --window then works on (cell, energy group) bins\n");
      }
      window_groups = nedges - 1;
      ++i;
    } else if (strcmp(argv[i], "--window-block") == 0) {
      /* one or two integers >= 1, nothing after them */
      char* end = NULL;
      const char* q = (i + 1 < argc) ? argv[i + 1] : "";
      const long bx = strtol(q, &end, 10);
      int ok = end != q && bx >= 1 && bx <= 0x7fffffffl && (*end == ',' || *end == '\0');
      long by = bx;
      if (ok && *end == ',') {
        q = end + 1;
        by = strtol(q, &end, 10);
        ok = end != q && by >= 1 && by <= 0x7fffffffl && *end == '\0';
      }
      if (!ok) {
        TERMINATE("--window-block wants BX[,BY], integers >= 1: --window then works on blocks of BX by BY "
                  "cells\n");
      }
      window_block_x = (int)bx;
      window_block_y = (int)by;
      ++i;
    } else if (strcmp(argv[i], "--batches") == 0) {
      char* end = NULL;
      const long b = (i + 1 < argc) ? strtol(argv[i + 1], &end, 10) : 0;
      if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || b < 2 || b > 1000000) {
        TERMINATE("--batches wants B >= 2 that divides the particle count: B independent batches of "
                  "N / B particles\n");
      }
      batches = (int)b;
      ++i;
    } else if (strcmp(argv[i], "--spectrum") == 0 && i + 1 < argc) {
      const char* spec = argv[++i];
      const char* at = strchr(spec, '@');
      spectrum_groups = -1;
      for (const char* q = spec; q && *q && q != at && spectrum_groups < 64;) {
        char* end = NULL;
        spectrum_edges[++spectrum_groups] = strtod(q, &end);
        if (end == q) {
          TERMINATE("--spectrum wants E0,E1,...,EG[@X0,Y0,X1,Y1]\n");
        }
        q = (*end == ',') ? end + 1 : end;
      }
      if (spectrum_groups < 1 ||
          (at && sscanf(at + 1, "%d,%d,%d,%d", &spectrum_box[0], &spectrum_box[1], &spectrum_box[2],
                        &spectrum_box[3]) != 4)) {
        TERMINATE("--spectrum wants E0,E1,...,EG[@X0,Y0,X1,Y1] with 1 to 64 groups\n");
      }
    } else if (strcmp(argv[i], "--leakage") == 0) {
      const char* spec = (i + 1 < argc) ? argv[++i] : "";
      char* end = NULL;
      const long m = strtol(spec, &end, 10);
      int nedges = 0, bad = (end == spec || m < 1 || m > 64);
      while (!bad && *end == ',') {
        const char* q = end + 1;
        const double e = strtod(q, &end);
        bad = (end == q || nedges > 64);
        if (!bad) {
          leakage_edges[nedges++] = e;
        }
      }
      if (bad || *end != '\0' || nedges == 1) {
        TERMINATE("--leakage wants M[,E0,E1,...,EG]: 1 to 64 cosine bins, then no edges or those of 1 to 64 "
                  "energy groups\n");
      }
      leakage_cosines = (int)m;
      leakage_groups = nedges ? nedges - 1 : 0;
    } else if (strcmp(argv[i], "--variant") == 0 && i + 1 < argc) {
      if (neutral_hip_set_variant(atoi(argv[++i]))) {
        TERMINATE("unknown --variant\n");
      }
    } else {
      TERMINATE("unknown argument %s\n", argv[i]);
    }
  }

  if (leakage_cosines && !vacuum_sides) {
    TERMINATE("--leakage needs --vacuum SIDES: nothing leaks through a wall that reflects\n");
  }

  if (bank_capacity && !vacuum_sides) {
    TERMINATE("--escape-bank needs --vacuum SIDES: nothing leaves through a wall that reflects\n");
  }
  if ((bank_capacity || source_bank_path[0]) && decompose_x) {
    TERMINATE("--escape-bank and --source-bank do not work with --decompose: a decomposed store keeps no bank "
              "and takes no source\n");
  }
  if (source_bank_path[0] && !source_count) {
    TERMINATE("--source-bank needs --source COUNT[,WEIGHT]: it says where those particles come from\n");
  }
  if (source_bank_path[0] && (source_file || source_mesh_file)) {
    TERMINATE("--source-bank does not work with --source-file or --source-mesh: one source or the other\n");
  }

  if (comb_every && decompose_x) {
    TERMINATE("--comb does not work with --decompose: a decomposed store cannot be combed\n");
  }

  if (source_count && decompose_x) {
    TERMINATE("--source does not work with --decompose: a decomposed store takes no source\n");
  }

  if (source_file && !source_count) {
    TERMINATE("--source-file needs --source COUNT[,WEIGHT]: it says where those particles come from\n");
  }
  if (source_mesh_file && !source_count) {
    TERMINATE("--source-mesh needs --source COUNT[,WEIGHT]: it says where those particles come from\n");
  }
  if (source_mesh_file && source_file) {
    TERMINATE("--source-mesh does not work with --source-file: one source or the other\n");
  }
  if (source_file) {
    read_source_file(source_file, source_components, &source_ncomponents, source_bins, &source_nbins);
  }

  if (window_in_step && !window) {
    TERMINATE("--window-in-step needs --window WLOW|auto[,UPPER_RATIO[,SURVIVAL_RATIO]]: it puts that window's "
              "lower bounds in force during the steps\n");
  }
  if (window && decompose_x && (!window_in_step || window_auto)) {
    TERMINATE("--window does not work with --decompose: a decomposed store takes no window (--window WLOW "
              "--window-in-step does: its bounds then play during the steps only)\n");
  }
  if (window_groups && !window) {
    TERMINATE("--window-groups needs --window WLOW|auto[,UPPER_RATIO[,SURVIVAL_RATIO]]: it says what bins "
              "that window works on\n");
  }

  if (window_block_x && !window) {
    TERMINATE("--window-block needs --window WLOW|auto[,UPPER_RATIO[,SURVIVAL_RATIO]]: it says what bins "
              "that window works on\n");
  }

  if (batches && decompose_x) {
    TERMINATE("--batches does not work with --decompose: a decomposed store is not run in batches\n");
  }

  /* deck actually read: the original, or a patched copy (one per rank) */
  char patched[4096];
  const char* read_deck = deck;
  if (noverrides) {
    snprintf(patched, sizeof(patched), "/tmp/neutral_hip_deck_%ld.params", (long)getpid());
    write_patched_deck(deck, patched, noverrides, keys, values);
    read_deck = patched;
  }

  Mesh mesh;
  memset(&mesh, 0, sizeof(mesh));
  mesh.global_nx = get_int_parameter("nx", read_deck);
  mesh.global_ny = get_int_parameter("ny", read_deck);
  if (source_mesh_file) {
    source_mesh_host = read_source_mesh_file(source_mesh_file, mesh.global_nx, mesh.global_ny);
  }
  mesh.pad = 0;
  mesh.local_nx = mesh.global_nx + 2 * mesh.pad;
  mesh.local_ny = mesh.global_ny + 2 * mesh.pad;
  mesh.width = 1.0;
  mesh.height = 1.0;
  mesh.sim_end = 1.0e30;
  (void)try_get_double_parameter("width", arch_params, &mesh.width);
  (void)try_get_double_parameter("height", arch_params, &mesh.height);
  (void)try_get_double_parameter("sim_end", arch_params, &mesh.sim_end);
  mesh.dt = get_double_parameter("dt", read_deck);
  mesh.niters = get_int_parameter("iterations", read_deck);
  mesh.rank = MASTER;
  mesh.nranks = 1;
  mesh.ndims = 2;
  if (batches && get_int_parameter("nparticles", read_deck) % batches != 0) {
    TERMINATE("--batches wants B >= 2 that divides the particle count: %d does not divide %d\n", batches,
              get_int_parameter("nparticles", read_deck));
  }

  initialise_mpi(argc, argv, &mesh.rank, &mesh.nranks);
  if (batches && mesh.nranks > 1) {
    TERMINATE("--batches does not work with several ranks: a batch is not sharded over ranks\n");
  }
  const int master = (mesh.rank == MASTER);
  if (master) {
    printf("Starting up with %d rank(s), one per GPU, kernel set: libneutral_hip (gfx950).\n",
           mesh.nranks);
    printf("Loading problem from %s.\n", deck);
  } else {
    neutral_hip_set_quiet(1); /* one "Particles" line per step: rank 0's */
  }
  initialise_devices(mesh.rank); /* binds the rank to its GPU, starts the tally exchange */
  initialise_comms(&mesh);
  if (decompose_x) {
    /* this rank's block of the mesh instead of all of it */
    int xo, yo, lx, ly;
    if (neutral_hip_set_decomposition(decompose_x, decompose_y, mesh.global_nx, mesh.global_ny,
                                      &xo, &yo, &lx, &ly)) {
      TERMINATE("--decompose %dx%d does not fit %d rank(s) and a %d x %d mesh.\n", decompose_x,
                decompose_y, mesh.nranks, mesh.global_nx, mesh.global_ny);
    }
    mesh.x_off = xo;
    mesh.y_off = yo;
    mesh.local_nx = lx + 2 * mesh.pad;
    mesh.local_ny = ly + 2 * mesh.pad;
  }
  initialise_mesh_2d(&mesh);
  SharedData shared_data = {0};
  initialise_shared_data_2d(mesh.local_nx, mesh.local_ny, mesh.pad, mesh.width, mesh.height,
                            read_deck, mesh.edgex, mesh.edgey, &shared_data);
  handle_boundary_2d(mesh.local_nx, mesh.local_ny, &mesh, shared_data.density, NO_INVERT, PACK);

  /* source box and particle count: four edge scalars come back from HBM */
  const int nx = mesh.local_nx - 2 * mesh.pad;
  const int ny = mesh.local_ny - 2 * mesh.pad;
  double edges[4];
  double* h = NULL;
  allocate_host_data(&h, 1);
  /* (the edge arrays hold this rank's edges: local indices) */
  double* d_edge[4] = {&mesh.edgex[mesh.pad], &mesh.edgey[mesh.pad], &mesh.edgex[nx + mesh.pad],
                       &mesh.edgey[ny + mesh.pad]};
  for (int k = 0; k < 4; ++k) {
    copy_buffer(1, &d_edge[k], &h, RECV);
    edges[k] = *h;
  }
  deallocate_host_data(h);
  if (decompose_x) {
    /* the library makes every rank look at all source particles and keep those of its
     * block: it wants the source box of the whole mesh */
    edges[0] = 0.0;
    edges[1] = 0.0;
    edges[2] = mesh.width;
    edges[3] = mesh.height;
  }
  NeutralSource src;
  neutral_source_from_deck(read_deck, mesh.width, mesh.height, edges[0], edges[1], edges[2],
                           edges[3], &src);

  if (decompose_x) {
    neutral_hip_set_source_box(src.local_particle_left_off, src.local_particle_bottom_off,
                               src.local_particle_width, src.local_particle_height);
  }
  double* tally = NULL;
  size_t allocation = allocate_data(&tally, (size_t)nx * (size_t)ny);
  double* collisions = NULL;
  double* absorbed = NULL;
  if (collision_tallies) {
    allocation += allocate_data(&collisions, (size_t)nx * (size_t)ny);
    allocation += allocate_data(&absorbed, (size_t)nx * (size_t)ny);
    neutral_hip_set_collision_tallies(collisions, absorbed);
  }
  double* current_meshes[3] = {NULL, NULL, NULL}; /* Jx, Jy and the scalar flux |J| is measured by */
  if (current) {
    for (int k = 0; k < 3; ++k) {
      allocation += allocate_data(&current_meshes[k], (size_t)nx * (size_t)ny);
    }
    neutral_hip_set_current_tally(current_meshes[0], current_meshes[1]);
    neutral_hip_set_scalar_flux_tally(current_meshes[2]);
  }
  double* outflow_meshes = NULL; /* west, east, south, north: one buffer */
  if (outflow) {
    allocation += allocate_data(&outflow_meshes, 4 * (size_t)nx * (size_t)ny);
    neutral_hip_set_outflow_tally(outflow_meshes);
  }
  double* leakage = NULL; /* the weights over N, then the counts: [side][group, no group last][cosine] */
  const size_t leakage_bins = 4 * (size_t)(leakage_groups + 1) * (size_t)leakage_cosines;
  if (leakage_cosines) {
    allocation += allocate_data(&leakage, 2 * leakage_bins);
    if (neutral_hip_set_leakage_tally(leakage_groups, leakage_groups ? leakage_edges : NULL, leakage_cosines,
                                      leakage) != 0) {
      TERMINATE("--leakage refused: finite, positive, strictly ascending edges\n");
    }
  }
  double* bank = NULL; /* [device] bank_capacity records of 64 bytes */
  if (bank_capacity) {
    if (bank_capacity > (1ull << 40)) {
      TERMINATE("--escape-bank: a bank of more than 2^40 records\n");
    }
    allocation += allocate_data(&bank, 8 * (size_t)bank_capacity);
    if (neutral_hip_set_escape_bank((NeutralHipEscapeRecord*)bank, bank_capacity) != 0) {
      TERMINATE("--escape-bank refused\n");
    }
  }
  double* source_bank = NULL; /* [device] the records of --source-bank */
  uint64_t source_bank_count = 0, source_bank_next = 0;
  if (source_bank_path[0]) {
    if (mesh.nranks > 1) {
      snprintf(source_bank_path + strlen(source_bank_path), 16, ".%d", mesh.rank);
    }
    FILE* f = fopen(source_bank_path, "rb");
    char magic[8];
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "NHBANK01", 8) != 0 ||
        fread(&source_bank_count, 8, 1, f) != 1 || source_bank_count > (1ull << 40)) {
      TERMINATE("--source-bank %s: not a bank file (NHBANK01, a count, the records)\n", source_bank_path);
    }
    double* h_records = NULL;
    allocate_host_data(&h_records, 8 * (size_t)source_bank_count);
    if (fread(h_records, 64, (size_t)source_bank_count, f) != (size_t)source_bank_count) {
      TERMINATE("--source-bank %s: fewer records than its count says\n", source_bank_path);
    }
    fclose(f);
    allocation += allocate_data(&source_bank, 8 * (size_t)(source_bank_count ? source_bank_count : 1));
    if (source_bank_count) {
      copy_buffer(8 * (size_t)source_bank_count, &h_records, &source_bank, SEND);
    }
    deallocate_host_data(h_records);
  }
  double* spectrum = NULL;
  if (spectrum_groups > 0) {
    if (spectrum_box[2] < 0) { /* (no box given: the whole mesh) */
      spectrum_box[2] = mesh.global_nx;
      spectrum_box[3] = mesh.global_ny;
    }
    if (spectrum_box[2] > mesh.global_nx || spectrum_box[3] > mesh.global_ny) {
      TERMINATE("--spectrum box lies outside the %d x %d mesh\n", mesh.global_nx, mesh.global_ny);
    }
    allocation += allocate_data(&spectrum, 2 * (size_t)spectrum_groups);
    if (neutral_hip_set_spectrum_tally(spectrum_groups, spectrum_edges, spectrum_box[0], spectrum_box[1],
                                       spectrum_box[2], spectrum_box[3], spectrum) != 0) {
      TERMINATE("--spectrum refused: finite, positive, strictly ascending edges and a non-empty box\n");
    }
  }
  if (window) {
    /* (with --window-groups: G meshes back to back, every bin's bound WLOW; with --window-block: the
     * coarse mesh's bins) */
    if (window_block_x) {
      window_cnx = (int)(((long long)mesh.global_nx + window_block_x - 1) / window_block_x);
      window_cny = (int)(((long long)mesh.global_ny + window_block_y - 1) / window_block_y);
    } else {
      window_cnx = mesh.global_nx;
      window_cny = mesh.global_ny;
    }
    const size_t ncells = (size_t)window_cnx * (size_t)window_cny * (size_t)(window_groups ? window_groups : 1);
    if (window_groups && ncells > 0x3fffffffull) {
      TERMINATE("--window-groups: the mesh has too many cells for %d groups\n", window_groups);
    }
    double* h_lower = NULL;
    allocate_host_data(&h_lower, ncells);
    for (size_t c = 0; c < ncells; ++c) {
      h_lower[c] = window_low;
    }
    allocation += allocate_data(&window_lower, ncells);
    copy_buffer(ncells, &h_lower, &window_lower, SEND);
    deallocate_host_data(h_lower);
    if (window_auto) {
      allocation += allocate_data(&window_census, 2 * ncells);
    }
    if (window_in_step &&
        neutral_hip_set_window_roulette(mesh.global_nx, mesh.global_ny, window_lower, window_survival, window_groups,
                                        window_groups ? window_edges : NULL, window_block_x ? window_block_x : 1,
                                        window_block_x ? window_block_y : 1) != 0) {
      TERMINATE("--window-in-step refused: it does not work with --roulette (one cutoff or the window's mesh)\n");
    }
  }
  if (source_mesh_file) {
    const size_t ncells = (size_t)mesh.global_nx * (size_t)mesh.global_ny;
    allocation += allocate_data(&source_mesh, ncells);
    copy_buffer(ncells, &source_mesh_host, &source_mesh, SEND);
    deallocate_host_data(source_mesh_host);
  }
  const int per_batch = batches ? src.nparticles / batches : 0;
  if (batches) {
    allocation += allocate_data(&batch_moments, 2 * (size_t)nx * (size_t)ny);
    allocation += allocate_data(&batch_relerr, (size_t)nx * (size_t)ny);
    neutral_hip_set_pid_base(0); /* the first batch: ids 0 .. N / B - 1 */
  }
  NeutralHipParticle* particles = NULL;
  int nlocal = batches ? per_batch : src.nlocal_particles;
  if (nlocal) {
    allocation += inject_particles(batches ? per_batch : src.nparticles, mesh.global_nx, mesh.local_nx, mesh.local_ny,
                                   mesh.pad, src.local_particle_left_off,
                                   src.local_particle_bottom_off, src.local_particle_width,
                                   src.local_particle_height, mesh.x_off, mesh.y_off, mesh.dt,
                                   mesh.edgex, mesh.edgey, src.initial_energy, &particles);
    if (decompose_x) {
      nlocal = neutral_hip_store_count(particles); /* what the source put into this block */
    }
  }
  /* fewer particles than ranks: this rank's shard is empty.  It makes the collective census call
   * like the others; the calls on its own shard (source, comb, window) have nothing to do */
  const int shard_empty = particles && !decompose_x && neutral_hip_store_count(particles) == 0;
  if (master) {
    printf("Allocated %.4fGB of data.\n", allocation / GB); /* neutral_data.c:117 */
  }

  NeutralHipCrossSection cs_scatter, cs_absorb;
  char path[4096];
  snprintf(path, sizeof(path), "%s/elastic_scatter.cs", cs_dir); /* neutral_data.h:30 */
  load_table(path, &cs_scatter);
  snprintf(path, sizeof(path), "%s/capture.cs", cs_dir); /* neutral_data.h:31 */
  load_table(path, &cs_absorb);

  /* timestep loop, main.c:85-147 */
  neutral_hip_set_lazy_export(1); /* nothing reads the particle arrays between steps */
  double wallclock = 0.0;
  double elapsed_sim_time = 0.0;
  int tt;
  /* --batches: the B batches one after the other, each through all its timesteps; the totals of the
   * batches' energy deposition, each times B an estimate of the run's, by Welford's update */
  double batch_mean = 0.0, batch_m2 = 0.0;
  const double batches_t0 = now_seconds();
  for (int batch = 0; batch < (batches ? batches : 1); ++batch) {
    if (batches) {
      if (master) {
        printf("\nBatch %d of %d\n", batch + 1, batches);
      }
      neutral_hip_set_pid_base((uint64_t)batch * (uint64_t)per_batch);
      if (batch > 0) {
        neutral_hip_reinject_particles(per_batch, mesh.local_nx, mesh.local_ny, mesh.pad,
                                       src.local_particle_left_off, src.local_particle_bottom_off,
                                       src.local_particle_width, src.local_particle_height, mesh.x_off,
                                       mesh.y_off, mesh.dt, mesh.edgex, mesh.edgey, src.initial_energy,
                                       particles);
      }
      neutral_hip_memset(tally, 0, sizeof(double) * (size_t)nx * (size_t)ny);
      elapsed_sim_time = 0.0;
    }
    for (tt = 1; tt <= mesh.niters; ++tt) {
      if (master) {
        printf("\nIteration  %d\n", tt); /* main.c:87-89 */
      }
      if (source_count && tt >= 2 && particles && !shard_empty) {
        /* (several ranks: each emits its share of COUNT into its own shard) */
        long long share_first = 0, share = source_count;
        if (mesh.nranks > 1) {
          comms_shard_range(source_count, mesh.rank, mesh.nranks, &share_first, &share);
        }
        if (source_bank_path[0]) {
          /* (every rank its own file, so every rank the whole COUNT; nothing is left: nothing is emitted) */
          const uint64_t left = source_bank_count - source_bank_next;
          const int take = left < (uint64_t)source_count ? (int)left : source_count;
          NeutralHipBankSourceStats bs;
          if (neutral_hip_source_bank(particles, nlocal, (const NeutralHipEscapeRecord*)source_bank, source_bank_next,
                                      take, source_weight, NULL, source_bank_snap, mesh.local_nx, mesh.local_ny,
                                      mesh.pad, mesh.x_off, mesh.y_off, mesh.dt, mesh.edgex, mesh.edgey, &bs) != 0) {
            TERMINATE("The bank source was refused (first bad record %llu).\n", (unsigned long long)bs.first_bad);
          }
          source_bank_next += bs.emitted;
          source_emitted += bs.emitted;
          source_weight_emitted += bs.weight_emitted;
        } else if (source_file) {
          NeutralHipDescribedSourceStats ds;
          if (neutral_hip_source_described(particles, nlocal, (int)share, source_weight,
                                           (1ull << 63) + (uint64_t)tt, source_ncomponents,
                                           source_components, source_nbins, source_bins, mesh.local_nx,
                                           mesh.local_ny, mesh.pad, mesh.x_off, mesh.y_off, mesh.dt,
                                           mesh.edgex, mesh.edgey, &ds) != 0) {
            TERMINATE("The described source was refused.\n");
          }
          source_emitted += ds.emitted;
          source_weight_emitted += ds.weight_emitted;
          for (int k = 0; k < source_ncomponents; ++k) {
            source_by_component[k] += ds.emitted_by_component[k];
          }
        } else if (source_mesh_file) {
          const NeutralHipSourceBin line = {src.initial_energy, src.initial_energy, 1.0};
          NeutralHipMeshSourceStats ms;
          if (neutral_hip_source_mesh(particles, nlocal, (int)share, source_weight,
                                      (1ull << 63) + (uint64_t)tt, source_mesh, 0.0, 2.0 * M_PI, 1, &line,
                                      mesh.local_nx, mesh.local_ny, mesh.pad, mesh.x_off, mesh.y_off, mesh.dt,
                                      mesh.edgex, mesh.edgey, &ms) != 0) {
            TERMINATE("The mesh source was refused.\n");
          }
          source_emitted += ms.emitted;
          source_weight_emitted += ms.weight_emitted;
          source_mesh_cells = ms.cells_nonzero;
        } else {
          NeutralHipSourceStats ss;
          if (neutral_hip_source_particles(particles, nlocal, (int)share, source_weight,
                                           (1ull << 63) + (uint64_t)tt, mesh.local_nx, mesh.local_ny,
                                           mesh.pad, src.local_particle_left_off,
                                           src.local_particle_bottom_off, src.local_particle_width,
                                           src.local_particle_height, mesh.x_off, mesh.y_off, mesh.dt,
                                           mesh.edgex, mesh.edgey, src.initial_energy, &ss) != 0) {
            TERMINATE("The source was refused.\n");
          }
          source_emitted += ss.emitted;
          source_weight_emitted += ss.weight_emitted;
        }
      }
      uint64_t facet_events = 0;
      uint64_t collision_events = 0;
      const double t0 = now_seconds();
      solve_transport_2d(nx, ny, mesh.global_nx, mesh.global_ny, (uint64_t)tt, mesh.pad,
                         mesh.x_off, mesh.y_off, mesh.dt, src.nparticles, &nlocal,
                         mesh.neighbours, particles, shared_data.density, mesh.edgex, mesh.edgey,
                         mesh.edgedx, mesh.edgedy, &cs_scatter, &cs_absorb, tally, NULL, NULL,
                         NULL, &facet_events, &collision_events);
      barrier();
      const double step_time = now_seconds() - t0;
      wallclock += step_time;
      if (master) {
        /* (event counts are the sums over all ranks) */
        if (vacuum_sides) {
          /* (behind the library's `Particles` line: the step's escapes by side, their weight) */
          NeutralHipEscapeStats es;
          neutral_hip_last_escape(&es);
          printf("Escaped  west %llu (%.9g) east %llu (%.9g) south %llu (%.9g) north %llu (%.9g)\n",
                 (unsigned long long)es.escaped[0], es.weight[0], (unsigned long long)es.escaped[1], es.weight[1],
                 (unsigned long long)es.escaped[2], es.weight[2], (unsigned long long)es.escaped[3], es.weight[3]);
        }
        if (periodic_axes) {
          /* (likewise: the step's wraps by the side left through, their weight) */
          NeutralHipWrapStats ws;
          neutral_hip_last_wraps(&ws);
          printf("Wrapped  west %llu (%.9g) east %llu (%.9g) south %llu (%.9g) north %llu (%.9g)\n",
                 (unsigned long long)ws.wrapped[0], ws.weight[0], (unsigned long long)ws.wrapped[1], ws.weight[1],
                 (unsigned long long)ws.wrapped[2], ws.weight[2], (unsigned long long)ws.wrapped[3], ws.weight[3]);
        }
        if (bank_capacity) {
          /* (this rank's own bank: every rank keeps one) */
          NeutralHipEscapeBankStats bk;
          neutral_hip_escape_bank_stats(&bk);
          printf("Banked: %llu %llu\n", (unsigned long long)bk.claimed, (unsigned long long)bk.recorded);
        }
        printf("Step time  %.4fs\n", step_time);
        printf("Wallclock  %.4fs\n", wallclock);
        printf("Facets     %llu\n", (unsigned long long)facet_events);
        printf("Collisions %llu\n", (unsigned long long)collision_events);
        printf("Facet Events / s %.2e\n", facet_events / step_time);
        printf("Collision Events / s %.2e\n", collision_events / step_time);
        NeutralHipStepStats st;
        neutral_hip_last_step(&st);
        printf("Particle-steps / s %.3e (facets + collisions + census, kernels %.2f ms)\n",
               (double)(st.facets + st.collisions + st.census) / step_time, st.kernel_ms);
        roulette_killed += st.roulette_killed; /* (summed over the ranks already) */
        roulette_survived += st.roulette_survived;
      }
      if (comb_every && tt % comb_every == 0 && particles && !shard_empty) {
        /* (several ranks: each combs its own shard; rank 0 reports its own) */
        NeutralHipCombStats cs;
        if (neutral_hip_comb_particles(particles, nlocal, (uint64_t)tt, &cs) == 0) {
          comb_min_live = (combs == 0 || cs.live_before < comb_min_live) ? cs.live_before : comb_min_live;
          comb_max_copies = (cs.max_copies > comb_max_copies) ? cs.max_copies : comb_max_copies;
          combs++;
        } else if (master) {
          printf("Comb refused: nothing live\n");
        }
      }
      /* (a decomposed store takes no census window: --window-in-step alone plays there) */
      if (window && !decompose_x && tt < mesh.niters && elapsed_sim_time + mesh.dt < mesh.sim_end && particles) {
        /* (several ranks: each windows its own shard) */
        int skip = 0;
        if (window_auto) {
          /* the census is collective and its meshes, hence the bounds, are the same on every rank;
           * the target is the live count over the ranks */
          NeutralHipCensusStats cs;
          double inside = 0.0; /* with groups: the live histories in one of them, the bounds' target */
          int census_rc;
          if (window_groups || window_block_x) {
            NeutralHipGroupCensusStats gs;
            if (window_block_x) {
              NeutralHipBlockCensusStats bs;
              census_rc = neutral_hip_census_tally_blocks(particles, nlocal, mesh.global_nx, mesh.global_ny,
                                                          window_block_x, window_block_y, window_groups,
                                                          window_groups ? window_edges : NULL, window_census, &bs);
              gs = bs.census;
            } else {
              census_rc = neutral_hip_census_tally_groups(particles, nlocal, mesh.global_nx, mesh.global_ny,
                                                          window_groups, window_edges, window_census, &gs);
            }
            cs.live = gs.live;
            cs.occupied_cells = gs.occupied_bins;
            cs.max_count = gs.max_count;
            cs.max_cell_weight = gs.max_bin_weight;
            inside = (double)(gs.live - gs.outside);
            window_outside += census_rc == 0 ? gs.outside : 0; /* (counted here: a skipped window counts none) */
          } else {
            census_rc = neutral_hip_census_tally(particles, nlocal, mesh.global_nx, mesh.global_ny, window_census,
                                                 &cs);
          }
          if (census_rc > 1) {
            TERMINATE("The census was refused.\n");
          }
          double live = (double)cs.live; /* (over the ranks: far below 2^53) */
          if (mesh.nranks > 1) {
            live = reduce_all_sum(live);
            inside = window_groups ? reduce_all_sum(inside) : inside;
          }
          skip = census_rc != 0;
          if (!skip) {
            if (master) {
              printf("Census live %.0f occupied %llu max_count %llu max_weight %.15e\n", live,
                     (unsigned long long)cs.occupied_cells, (unsigned long long)cs.max_count,
                     cs.max_cell_weight);
            }
            /* (G meshes back to back are one of nx by G * ny: the same call makes the bins' bounds) */
            const int bounds_rc = neutral_hip_window_bounds(
                window_cnx, window_cny * (window_groups ? window_groups : 1), window_census,
                window_groups ? inside : live, window_upper, 0.0, 1, window_lower, NULL);
            if (bounds_rc > 1) {
              TERMINATE("The bounds were refused.\n");
            }
            skip = bounds_rc != 0;
          }
          window_skipped += skip;
        }
        NeutralHipWindowStats ws;
        memset(&ws, 0, sizeof(ws));
        if (!skip && !shard_empty && (window_groups || window_block_x)) {
          NeutralHipGroupWindowStats gs;
          const int window_rc =
              window_block_x
                  ? neutral_hip_window_particles_blocks(particles, nlocal, mesh.global_nx, mesh.global_ny,
                                                        window_block_x, window_block_y, window_groups,
                                                        window_groups ? window_edges : NULL, window_lower,
                                                        window_upper, window_survival, window_max_split,
                                                        (3ull << 62) + (uint64_t)tt, &gs)
                  : neutral_hip_window_particles_groups(particles, nlocal, mesh.global_nx, mesh.global_ny,
                                                        window_groups, window_edges, window_lower, window_upper,
                                                        window_survival, window_max_split,
                                                        (3ull << 62) + (uint64_t)tt, &gs);
          if (window_rc != 0) {
            TERMINATE("The window was refused.\n");
          }
          ws = gs.window;
          window_outside += window_auto ? 0 : gs.outside;
        } else if (!skip && !shard_empty &&
                   neutral_hip_window_particles(particles, nlocal, mesh.global_nx, mesh.global_ny, window_lower,
                                                window_upper, window_survival, window_max_split,
                                                (3ull << 62) + (uint64_t)tt, &ws) != 0) {
          TERMINATE("The window was refused.\n");
        }
        window_totals[0] += ws.roulette_killed;
        window_totals[1] += ws.roulette_survived;
        window_totals[2] += ws.split;
        window_totals[3] += ws.copies_made;
        window_totals[4] += ws.copies_refused;
      }
      elapsed_sim_time += mesh.dt;
      if (elapsed_sim_time >= mesh.sim_end) {
        if (master) {
          printf("Reached end of simulation time\n");
        }
        break;
      }
    }
    if (batches) {
      NeutralHipBatchFoldStats fs;
      if (neutral_hip_batch_fold(tally, (size_t)nx * (size_t)ny, batch + 1, batch_moments, &fs) != 0) {
        TERMINATE("The batch's tally was refused: an entry is not finite.\n");
      }
      const double total = fs.sum * (double)batches;
      const double d = total - batch_mean;
      batch_mean = batch_mean + d / (double)(batch + 1);
      const double d2 = total - batch_mean;
      batch_m2 = batch_m2 + d * d2;
    }
  }
  NeutralHipBatchStats batch_stats;
  double batches_seconds = 0.0;
  if (batches) {
    /* the estimate of all the batches together takes the tally's place: it is what is validated */
    if (neutral_hip_batch_statistics(batch_moments, (size_t)nx * (size_t)ny, batches, (double)batches, tally,
                                     batch_relerr, &batch_stats) != 0) {
      TERMINATE("The batch statistics were refused.\n");
    }
    batches_seconds = now_seconds() - batches_t0;
  }

  neutral_hip_sync_particles(particles);
  validate(nx, ny, deck, mesh.rank, tally);
  if (collision_tallies) {
    /* totals over the mesh (a decomposed mesh: over every rank's block) */
    double* h_mesh = NULL;
    const size_t ncells = (size_t)nx * (size_t)ny;
    allocate_host_data(&h_mesh, ncells);
    double totals[2];
    double* meshes[2] = {collisions, absorbed};
    for (int k = 0; k < 2; ++k) {
      copy_buffer(ncells, &meshes[k], &h_mesh, RECV);
      totals[k] = 0.0;
      for (size_t c = 0; c < ncells; ++c) {
        totals[k] += h_mesh[c];
      }
      if (decompose_x) {
        totals[k] = reduce_all_sum(totals[k]);
      }
    }
    deallocate_host_data(h_mesh);
    if (master) {
      printf("Collision tally total %.0f\n", totals[0]);
      printf("Absorbed weight total %.12e\n", totals[1]);
    }
  }
  if (current) {
    /* totals over the mesh and the most beam-like cell, |J| / phi (a decomposed mesh: over every
     * rank's block) */
    const size_t ncells = (size_t)nx * (size_t)ny;
    double* h_meshes[3] = {NULL, NULL, NULL};
    for (int k = 0; k < 3; ++k) {
      allocate_host_data(&h_meshes[k], ncells);
      copy_buffer(ncells, &current_meshes[k], &h_meshes[k], RECV);
    }
    double sum_jx = 0.0, sum_jy = 0.0, max_ratio = 0.0;
    for (size_t c = 0; c < ncells; ++c) {
      sum_jx += h_meshes[0][c];
      sum_jy += h_meshes[1][c];
      if (h_meshes[2][c] > 0.0) {
        const double ratio =
            sqrt(h_meshes[0][c] * h_meshes[0][c] + h_meshes[1][c] * h_meshes[1][c]) / h_meshes[2][c];
        max_ratio = (ratio > max_ratio) ? ratio : max_ratio;
      }
    }
    if (decompose_x) {
      sum_jx = reduce_all_sum(sum_jx);
      sum_jy = reduce_all_sum(sum_jy);
      max_ratio = reduce_all_max(max_ratio);
    }
    for (int k = 0; k < 3; ++k) {
      deallocate_host_data(h_meshes[k]);
    }
    if (master) {
      printf("Current sum Jx %.12e sum Jy %.12e max |J|/phi %.12e\n", sum_jx, sum_jy, max_ratio);
    }
  }
  if (outflow) {
    /* the four sides summed over the mesh, and the outer boundary sides alone: the weight that
     * struck the mesh's walls (a decomposed mesh: over every rank's block) */
    const size_t ncells = (size_t)nx * (size_t)ny;
    double* h_out = NULL;
    allocate_host_data(&h_out, 4 * ncells);
    copy_buffer(4 * ncells, &outflow_meshes, &h_out, RECV);
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    double wall_hits = 0.0;
    for (int s = 0; s < 4; ++s) {
      for (int y = 0; y < ny; ++y) {
        for (int x = 0; x < nx; ++x) {
          const double v = h_out[(size_t)s * ncells + (size_t)y * (size_t)nx + (size_t)x];
          const int gx = mesh.x_off + x;
          const int gy = mesh.y_off + y;
          const int on_wall = (s == 0) ? (gx == 0) : (s == 1) ? (gx == mesh.global_nx - 1)
                              : (s == 2) ? (gy == 0) : (gy == mesh.global_ny - 1);
          sums[s] += v;
          wall_hits += on_wall ? v : 0.0;
        }
      }
    }
    deallocate_host_data(h_out);
    if (decompose_x) {
      for (int s = 0; s < 4; ++s) {
        sums[s] = reduce_all_sum(sums[s]);
      }
      wall_hits = reduce_all_sum(wall_hits);
    }
    if (master) {
      printf("Outflow west %.12e east %.12e south %.12e north %.12e\n", sums[0], sums[1], sums[2], sums[3]);
      printf("Outflow wall hits %.12e\n", wall_hits);
    }
  }
  if (spectrum_groups > 0) {
    /* (a decomposed mesh: every rank scored its own cells of the box) */
    double* h_spectrum = NULL;
    allocate_host_data(&h_spectrum, 2 * (size_t)spectrum_groups);
    copy_buffer(2 * (size_t)spectrum_groups, &spectrum, &h_spectrum, RECV);
    if (decompose_x) {
      for (int k = 0; k < 2 * spectrum_groups; ++k) {
        h_spectrum[k] = reduce_all_sum(h_spectrum[k]);
      }
    }
    if (master) {
      for (int k = 0; k < spectrum_groups; ++k) {
        printf("Spectrum group %d [%.6e, %.6e) track %.12e collision %.12e\n", k, spectrum_edges[k],
               spectrum_edges[k + 1], h_spectrum[k], h_spectrum[spectrum_groups + k]);
      }
    }
    deallocate_host_data(h_spectrum);
  }
  if (leakage_cosines) {
    /* (a decomposed mesh: the rank that owns a boundary cell scored its escapes) */
    static const char* const side_names[4] = {"west", "east", "south", "north"};
    double* h_leakage = NULL;
    allocate_host_data(&h_leakage, 2 * leakage_bins);
    copy_buffer(2 * leakage_bins, &leakage, &h_leakage, RECV);
    if (decompose_x) {
      for (size_t k = 0; k < 2 * leakage_bins; ++k) {
        h_leakage[k] = reduce_all_sum(h_leakage[k]);
      }
    }
    for (int s = 0; s < 4 && master; ++s) {
      if (!((vacuum_sides >> s) & 1u)) {
        continue;
      }
      double count = 0.0, weight = 0.0;
      for (int g = 0; g <= leakage_groups; ++g) {
        if (g < leakage_groups) {
          printf("Leakage %s group %d [%.6e, %.6e)", side_names[s], g, leakage_edges[g], leakage_edges[g + 1]);
        } else {
          printf("Leakage %s no group", side_names[s]);
        }
        for (int m = 0; m < leakage_cosines; ++m) {
          const size_t b = ((size_t)s * (size_t)(leakage_groups + 1) + (size_t)g) * (size_t)leakage_cosines + (size_t)m;
          printf(" %.12e", h_leakage[b]);
          weight += h_leakage[b];
          count += h_leakage[leakage_bins + b];
        }
        printf("\n");
      }
      /* (the weight in the units of the `Escaped` lines: the tally holds it over N) */
      printf("Leakage %s total %.0f (%.9g)\n", side_names[s], count, weight * (double)src.nparticles);
    }
    deallocate_host_data(h_leakage);
  }
  if (bank_capacity && bank_path) {
    NeutralHipEscapeBankStats bk;
    neutral_hip_escape_bank_stats(&bk);
    double* h_bank = NULL;
    allocate_host_data(&h_bank, 8 * (size_t)bk.recorded);
    if (bk.recorded) {
      copy_buffer(8 * (size_t)bk.recorded, &bank, &h_bank, RECV);
    }
    char path[4096 + 16];
    if (mesh.nranks > 1) {
      snprintf(path, sizeof(path), "%.4000s.%d", bank_path, mesh.rank);
    } else {
      snprintf(path, sizeof(path), "%.4000s", bank_path);
    }
    FILE* f = fopen(path, "wb");
    const uint64_t count = bk.recorded;
    if (!f || fwrite("NHBANK01", 1, 8, f) != 8 || fwrite(&count, 8, 1, f) != 1 ||
        fwrite(h_bank, 64, (size_t)count, f) != (size_t)count || fclose(f) != 0) {
      TERMINATE("--escape-bank: could not write %s\n", path);
    }
    deallocate_host_data(h_bank);
  }
  if ((roulette || window_in_step) && master) {
    printf("Roulette killed %llu\n", roulette_killed);
    printf("Roulette survived %llu\n", roulette_survived);
  }
  if (comb_every && master) {
    printf("Combs %d\n", combs);
    printf("Comb smallest live count %llu\n", comb_min_live);
    printf("Comb largest max_copies %llu\n", comb_max_copies);
  }
  if (source_count) {
    double emitted = (double)source_emitted; /* (over the ranks: far below 2^53) */
    if (mesh.nranks > 1) {
      emitted = reduce_all_sum(emitted);
      source_weight_emitted = reduce_all_sum(source_weight_emitted);
    }
    if (master) {
      printf("Source emitted %.0f\n", emitted);
      printf("Source weight emitted %.12e\n", source_weight_emitted);
    }
    for (int k = 0; k < source_ncomponents; ++k) {
      double by_component = (double)source_by_component[k];
      if (mesh.nranks > 1) {
        by_component = reduce_all_sum(by_component);
      }
      if (master) {
        printf("Source component %d emitted %.0f\n", k, by_component);
      }
    }
    if (source_mesh_file && master) {
      printf("Source mesh emitted %.0f from %llu cells\n", emitted, source_mesh_cells);
    }
  }
  if (window) {
    static const char* const names[5] = {"roulette killed", "roulette survived", "split", "copies made",
                                         "copies refused"};
    for (int k = 0; k < 5; ++k) {
      double total = (double)window_totals[k]; /* (over the ranks: far below 2^53) */
      if (mesh.nranks > 1) {
        total = reduce_all_sum(total);
      }
      if (master) {
        printf("Window %s %.0f\n", names[k], total);
      }
    }
    if (window_auto && master) {
      printf("Window auto skipped %d\n", window_skipped); /* (the same on every rank) */
    }
    if (window_block_x && master) {
      printf("Window blocks %d x %d\n", window_cnx, window_cny);
    }
    if (window_groups) {
      double outside = (double)window_outside; /* (over the ranks: far below 2^53) */
      if (mesh.nranks > 1) {
        outside = reduce_all_sum(outside);
      }
      if (master) {
        printf("Window outside %.0f\n", outside);
      }
    }
  }
  if (batches && master) {
    const double se = sqrt(batch_m2 / (double)(batches - 1) / (double)batches);
    const double r = batch_stats.mean_relerr;
    printf("Batches %d of %d particles\n", batches, per_batch);
    printf("Batch total energy deposition %.15e +- %.6e (relative %.6e)\n", batch_mean, se,
           batch_mean != 0.0 ? se / fabs(batch_mean) : 0.0);
    printf("Batch relative error mean %.6e max %.6e over %llu scored cells\n", r, batch_stats.max_relerr,
           (unsigned long long)batch_stats.scored);
    printf("Batch scored cells within 10%% %llu within 5%% %llu\n",
           (unsigned long long)batch_stats.within_10pc, (unsigned long long)batch_stats.within_5pc);
    printf("Batch FOM %.6e (1 / (mean relative error^2 * %.4fs))\n",
           r > 0.0 && batches_seconds > 0.0 ? 1.0 / (r * r * batches_seconds) : 0.0, batches_seconds);
  }
  if (master) {
    printf("Final Wallclock %.9fs\n", wallclock);
    printf("Elapsed Simulation Time %.6fs\n", elapsed_sim_time);
  }
  if (noverrides) {
    remove(patched);
  }
  barrier();
  neutral_hip_comm_stop();
  return 0;
}
