// options.hpp — the tuning options of a handle (mfea_set_option /
// mfea_get_option, include/mfea_debug.h): the values they store, with their
// defaults, and ONE descriptor per option name (options.cpp kOptions) that says
// how the value is read and written, which values are legal, and what setting
// it does to the handle beyond the field.  Plain C++, no device types: a new
// option is a field here and a row there.
#pragma once
#include <cstdint>

#include "amg.hpp"

namespace mfea {

constexpr int kOptSweepPieceMax = 64;  // = kSweepPieceLen (amg_kernels.hpp; asserted in capi.hip)
constexpr int kOptBigChunkMax = 63;    // = mfea_handle::kRemGraphs - 1 (asserted in capi.hip)

// Every value a writable option stores.  The initialisers are the defaults
// (the measured best; the library reads no environment variables).
struct Options {
  // option "phase_times": record the phase events (mfea_stats t_*_ms).  Off by
  // default: each event recorded between two kernels left the GPU idle for
  // ≈ 5–10 µs (C2 step 0.771 → 0.737 ms, C3 1.665 → 1.635 without them)
  bool opt_phase_times = false;
  // mfea_step, one partition (option "spec_post"): the post kernels and
  // their read-back are enqueued behind the solve's planned batch, before the
  // host waits for it, so the one wait covers both — one host round trip per
  // step instead of two.  spec_on: this step may; spec_launched: enqueued
  // behind the last batch (undone by k_unfail when the solve goes on)
  int opt_spec_post = 1;
  // the solve's entry launches (cg_init, first V-cycle, w, update 0) in the
  // captured setup graph (option "setup_entry")
  int opt_setup_entry = 1;
  // mfea_step, one partition, GAMG / SOR / ICC, graphs on, no phase events:
  // the planned batch, the finish and the post as one captured graph
  int opt_batch_graph = 1;
  // mfea_step likewise: the assembly with the fused RHS and the CG start
  // captured at the head of the setup graph, the grip displacements read from
  // pinned h_red[14..15] by a copy node (option "step_graph").  Off: measured
  // 13 µs slower per step at C2 and C3 (profiles/r6/ab_step_graph_wall.log) —
  // an eager assembly runs while the host checks the plan and the setup
  // graph's key; deferred, the GPU waits for that host work
  int opt_step_graph = 0;
  int opt_graph_start = 1;  // the CG start (k_cg_init_finalize) at the setup graph's head
  // with batch_graph: the batch, finish and post behind the setup in one graph
  int opt_combo_graph = 1;
  // One partition (option "keep_operator"): mfea_step keeps K
  // (val / diag) while what it was assembled from holds — the activity
  // (act_gen), the material, the build (`assembled`), the assembly kernel —
  // and solve_amg keeps the numeric setup's values while K (op_gen) and the
  // setup's other inputs hold (Part::kept).  None of them depends on the grip
  // displacements, the only thing that moves from one load step to the next.
  int opt_keep_operator = 1;
  // One-partition GAMG solves on the unpreconditioned norm end every chunk
  // with a closing check (enqueue_amg_chunk): the planned batch is one group
  // shorter, the converging update's V-cycle and w = A u are not run.  0: the
  // batch ends with the update that finds the convergence, as before.
  int opt_amg_close = 1;
  // A solve on kept hierarchy values starts with ONE launch (k_amg_start: the
  // RHS, the CG's state and level-0 b) instead of three.  0: the three.
  int opt_amg_start = 1;
  // The update moves s, r and level 0's x only; p and x are replayed from the
  // chunk's kept u at its end (amg_kernels.hpp AmgPx).  0: the fat update.
  int opt_amg_lazy_px = 1;
  int opt_event_scratch = 1;  // option "event_scratch": 1 the scan keeps ε_e for the apply, 0 it forms them again
  bool opt_graph = true;       // single-partition chunks replay as hipGraphs
  bool opt_dist_graph = true;  // partitioned chunks too
  int opt_order = kOrderDFS;   // free-row order (symbolic.hpp)
  int opt_lane_dof = 0;        // 0: 2 DOFs per node on planar meshes, 3: always 3
  int opt_cg_kernel = 0;       // Jacobi CG: 0 by density, 1 lanes, 2 SELL
  int opt_ell_block = 256;     // lane kernels: threads per block
  int64_t opt_ell_maxg = 0;    // lane kernels: grid cap (0: kCgMaxG)
  bool opt_ell_compact = true; // lane kernels: compact halo records
  int64_t opt_amg_tail_rows = 2048;  // GAMG: levels of at most this many rows run in one workgroup
  int opt_amg_max_levels = kAmgMaxLevels;  // GAMG: hierarchy depth cap
  int opt_amg_rlanes = 0;      // GAMG: restriction lanes per coarse row (0: by width)
  int opt_amg_down_split = 0;  // GAMG compact down sweep: R̂ and Ã rows as two launches (experiment)
  int opt_amg_merge = -1;      // GAMG: levels 0 and 1 merged around a level-2 collapse (-1: small networks, 0 off, 1 on)
  int opt_amg_v_lanes = 0;     // GAMG collapsed cycle: lanes per V row (0: by width; 1, 2, 4, 8, 16)
  int64_t opt_amg_small_lanes = 65536;  // GAMG: wide rows of small levels at 16 lanes below this many threads
  int opt_amg_alanes = 0;      // GAMG: operator lanes per row below level 0 (0: by width)
  int opt_amg_tail_lds = 1;    // GAMG: the single-workgroup tail keeps its vectors in LDS
  int opt_amg_collapse = -1;           // GAMG: collapse the compact cycle below the highest level
                                      // within budget (-1), never (0), or from level ≥ k (k ≥ 1)
  int64_t opt_amg_collapse_mb = 32;     // … budget: the collapsed operator's bytes
  int64_t opt_amg_collapse_pairs = 8000000;  // … budget: its setup products' list items
  int opt_amg_spatial = -1;  // GAMG: rows labelled in Z-order (1), depth-first (0), by locality (-1)
  int opt_amg_up_lanes = 0;  // GAMG compact up sweep: lanes per P̃ row (0: by width)
  // GAMG: level 0's last up sweep and w = A u as one launch over block-local
  // rows (k_amg_up_w): -1 by kAmgFuseAuto, 0 never, 1 where
  // the plan allows it.  amg_l0_window: level 0's sorting window in rows
  // (0: kAmgFuseWindow where the fusion is wanted, 4096 elsewhere)
  int opt_amg_fuse_l0 = -1;
  int64_t opt_amg_l0_window = 0;
  // GAMG: ρ̂ of the levels below 0 in ppm (ω_l = 4 / (3 ρ̂)); 0: max(2, g_l / 1.45), the
  // Gershgorin-safe value.  A solve that fails with it falls back to the safe
  // value for the handle's lifetime (amg_safe_omega, omega_fallback).
  int64_t opt_amg_coarse_rho_ppm = 1750000;
  int opt_amg_a0_slot = 1;  // level 0's blocks one thread per position (k_amg_a0slot) at a fixed ω
  int opt_amg_big_chunk = 8;  // GAMG: iterations per chunk of a planned batch (drive_sized)
  int opt_sweep_piece = kOptSweepPieceMax;  // SOR / ICC: rows per chain piece (amg.hpp SweepPlan)
  int opt_amg_fuse_setup = 1;  // GAMG setup: the compact operators fused into the Galerkin chain's launches
  int64_t opt_amg_theta_ppm = 0;  // GAMG: strength threshold θ·10⁶ of the level-0 aggregation (0: all strong)
  int opt_amg_cycle = 1;       // GAMG: 1 the compact V-cycle (two sweeps per level), 0 four steps
  double opt_part_slack = 0.35;  // partition boundaries: min-cut search window (fraction of a strip)
  // GAMG over element failures: 1 keep the hierarchy (floating pieces masked)
  // until a solve needs more than amg_rebuild_pct % of the iterations of the
  // hierarchy's first solve (+2), then rebuild; 0 rebuild on every new active set
  int opt_amg_reuse = 1;
  // assembly: 0 row gather (one launch, fused GAMG RHS), 1 element colours
  // (a launch per colour), 2 element pass + row pass (two launches)
  int opt_asm_kernel = 0;
  int opt_cc_tile = 1024;  // floating rows on the device: rows per LDS tile (512, 1024, 2048, 4096; C3 73 µs at 512-1024, C5 0.6 ms at 1024-2048)
  int opt_amg_rebuild_pct = 800;
  // ... or once the time its solves spent on iterations above that count
  // reaches this % of the time the last build took (0: off).  Rent-or-buy:
  // a C5 rebuild costs 2.4 s of host work — ≈ 80 steps — so a kept hierarchy
  // that needs 40-100 % more iterations is kept; at most twice the cost of
  // the best choice in hindsight (measured)
  int opt_amg_rebuild_rent = 100;
  int opt_amg_dist = -1;          // partitioned GAMG: 1 the global hierarchy (distributed V-cycle), 0 block
                                  // Jacobi over per-partition hierarchies, -1 whichever solves faster (measured)
  int64_t opt_amg_rep_rows = 32768;  // distributed V-cycle: levels of at most this many rows are replicated
  // distributed V-cycle: 1 the compact cycle with level 0 split and every
  // level below replicated (x_0 halo, x_1 all-gather, u halo: three exchange
  // points per iteration), 0 the four-step cycle over the levels of more than
  // amg_rep_rows rows (four exchange points per split level)
  int opt_amg_dist_cycle = 1;
  // GAMG over RCCL: the CG's per-rank partial sums as ONE ncclAllReduce of
  // [world][4] doubles, every rank's buffer zero but its own row (1; the sum
  // is then each row exactly, summed by every rank in rank order as before),
  // or as world − 1 send / receive pairs per rank (0)
  int opt_dist_sums = 1;
  bool opt_run_register = true;  // option "run_register": page-lock the caller's record arrays
  double dist_timeout_s = 60.0;  // per RCCL wait; option "dist_timeout_ms"
};

// Which values mfea_set_option takes for an option
struct OptLegal {
  enum Kind : uint8_t {
    kAny,          // every value
    kFlag,         // every value, stored as value != 0
    kRange,        // v[0] <= value <= v[1]
    kList,         // one of v[0..n)
    kZeroOrRange,  // 0, or v[0] <= value <= v[1]
    kWindow,       // 0, or a multiple of 64 up to v[0]
  } kind;
  int n;
  int64_t v[6];
};

// Whether setting the option keeps K and the hierarchy's values (option
// keep_operator): most options only change launches, but only those that
// cannot change a value say so.
enum class OptKeeps : uint8_t { kNo, kYes, kWhenSet /* to a value != 0 */ };

// What setting the option does beyond storing it (capi.hip option_effect)
enum class OptEffect : uint8_t {
  kNone,
  kLevelLanes,  // the per-level copies of the lane options (Part::amg_lev)
  kCycle,       // amg_cycle: the levels' form, uploaded
  kOmega,       // amg_coarse_rho_ppm: the fallback to the safe ω is forgotten
  kReuse,       // amg_reuse: the next solve builds for its own active set
  kDistAuto,    // amg_dist: the automatic choice starts over
  kGlobalPlan,  // amg_rep_rows, amg_dist_cycle: the global hierarchy is rebuilt
  kDistSums,    // dist_sums: the zero-padded exchange buffer
};

struct OptionDesc {
  const char* name;
  int64_t (*load)(const Options&);
  void (*store)(Options&, int64_t);
  OptLegal legal;
  const char* legal_text;  // for the error message
  bool rebuilds_layout;    // baked into the symbolic layout: rebuilt at the next call, the activity kept
  OptKeeps keeps_kept;
  OptEffect effect;
};

int option_count();
const OptionDesc& option_at(int i);
const OptionDesc* find_option(const char* name);  // nullptr: no writable option of that name
bool option_legal(const OptionDesc& d, int64_t value);
inline bool option_keeps(const OptionDesc& d, int64_t value) {
  return d.keeps_kept == OptKeeps::kYes || (d.keeps_kept == OptKeeps::kWhenSet && value != 0);
}
// value must be legal; a read-back then gives load(o)
void option_store(const OptionDesc& d, Options& o, int64_t value);
inline int64_t option_default(const OptionDesc& d) { return d.load(Options{}); }

}  // namespace mfea
