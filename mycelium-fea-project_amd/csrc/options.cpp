// options.cpp — the option table of options.hpp.
#include "options.hpp"

#include <cmath>
#include <cstring>
#include <type_traits>

namespace mfea {
namespace {

// a bool, int or int64_t field, through int64_t
template <auto M>
int64_t load(const Options& o) {
  return (int64_t)(o.*M);
}
template <auto M>
void store(Options& o, int64_t v) {
  o.*M = static_cast<std::remove_reference_t<decltype(o.*M)>>(v);
}
// a double field holding the option's value / Scale
template <auto M, int Scale>
int64_t load_scaled(const Options& o) {
  return (int64_t)std::llround(o.*M * (double)Scale);
}
template <auto M, int Scale>
void store_scaled(Options& o, int64_t v) {
  o.*M = v / (double)Scale;
}

constexpr OptLegal kAny{OptLegal::kAny, 0, {}};
constexpr OptLegal kFlag{OptLegal::kFlag, 0, {}};
constexpr OptLegal range(int64_t lo, int64_t hi) { return {OptLegal::kRange, 2, {lo, hi}}; }
constexpr OptLegal zero_or(int64_t lo, int64_t hi) { return {OptLegal::kZeroOrRange, 2, {lo, hi}}; }
constexpr OptLegal window(int64_t max) { return {OptLegal::kWindow, 1, {max}}; }
template <class... T>
constexpr OptLegal list(T... v) {
  return {OptLegal::kList, (int)sizeof...(T), {v...}};
}
constexpr OptLegal kBit = range(0, 1);

#define FIELD(m) load<&Options::m>, store<&Options::m>
#define SCALED(m, s) load_scaled<&Options::m, s>, store_scaled<&Options::m, s>
constexpr bool kLayout = true;
constexpr OptKeeps kDrops = OptKeeps::kNo, kKeeps = OptKeeps::kYes;
using E = OptEffect;

// name, field, legal values (and their text), rebuilds the layout, keeps the
// kept K / hierarchy values, effect
const OptionDesc kOptions[] = {
    {"graph", FIELD(opt_graph), kFlag, "0 or 1", false, kDrops, E::kNone},
    {"run_register", FIELD(opt_run_register), kFlag, "0 or 1", false, kKeeps, E::kNone},
    {"event_scratch", FIELD(opt_event_scratch), kFlag, "0 or 1", false, kDrops, E::kNone},
    {"phase_times", FIELD(opt_phase_times), kFlag, "0 or 1", false, kKeeps, E::kNone},
    {"dist_graph", FIELD(opt_dist_graph), kFlag, "0 or 1", false, kDrops, E::kNone},
    {"order", FIELD(opt_order), kAny, "-1 (DFS), 0 (natural) or a window", kLayout, kDrops, E::kNone},
    {"lane_dof", FIELD(opt_lane_dof), kAny, "0 or 3", kLayout, kDrops, E::kNone},
    {"cg_kernel", FIELD(opt_cg_kernel), range(0, 2), "0 auto, 1 lanes, 2 sell", false, kDrops, E::kNone},
    {"ell_block", FIELD(opt_ell_block), list(64, 128, 256, 512), "64, 128, 256 or 512", false, kDrops, E::kNone},
    {"ell_maxg", FIELD(opt_ell_maxg), kAny, "a grid cap (0: the default)", false, kDrops, E::kNone},
    {"ell_compact", FIELD(opt_ell_compact), kFlag, "0 or 1", kLayout, kDrops, E::kNone},
    {"amg_tail_rows", FIELD(opt_amg_tail_rows), kAny, "a row count (0: off)", kLayout, kDrops, E::kNone},
    {"amg_max_levels", FIELD(opt_amg_max_levels), range(1, kAmgMaxLevels), "1..32", kLayout, kDrops, E::kNone},
    {"amg_restrict_lanes", FIELD(opt_amg_rlanes), list(0, 1, 2, 4, 8, 16),
     "0 (by width), 1, 2, 4, 8 or 16 (16: the compact down sweep)", false, kDrops, E::kLevelLanes},
    {"amg_v_lanes", FIELD(opt_amg_v_lanes), list(0, 1, 2, 4, 8, 16), "0 (by width), 1, 2, 4, 8 or 16", false, kDrops,
     E::kLevelLanes},
    {"amg_small_lanes", FIELD(opt_amg_small_lanes), range(0, int64_t(1) << 30), "0 .. 2^30", false, kDrops,
     E::kLevelLanes},
    {"amg_merge", FIELD(opt_amg_merge), range(-1, 1), "-1 (small networks), 0 or 1", kLayout, kDrops, E::kNone},
    {"amg_down_split", FIELD(opt_amg_down_split), kFlag, "0 or 1", false, kDrops, E::kLevelLanes},
    {"amg_op_lanes", FIELD(opt_amg_alanes), list(0, 1, 2, 4), "0 (by width), 1, 2 or 4", false, kDrops,
     E::kLevelLanes},
    {"amg_tail_lds", FIELD(opt_amg_tail_lds), kFlag, "0 or 1", false, kDrops, E::kLevelLanes},
    {"amg_collapse", FIELD(opt_amg_collapse), range(-1, kAmgMaxLevels - 1),
     "-1 (within budget), 0 (off) or a level up to 31", kLayout, kDrops, E::kNone},
    {"amg_collapse_mb", FIELD(opt_amg_collapse_mb), range(0, int64_t(1) << 20), "0 .. 2^20 MB", kLayout, kDrops,
     E::kNone},
    {"amg_collapse_pairs", FIELD(opt_amg_collapse_pairs), range(0, INT32_MAX - 1), "0 .. 2^31 - 2", kLayout, kDrops,
     E::kNone},
    {"amg_spatial", FIELD(opt_amg_spatial), range(-1, 1), "-1 (by locality), 0 or 1", kLayout, kDrops, E::kNone},
    // (amg_fuse_l0's automatic choice also picks level 0's window)
    {"amg_fuse_l0", FIELD(opt_amg_fuse_l0), range(-1, 1), "-1 (auto), 0 or 1", kLayout, kDrops, E::kNone},
    {"amg_l0_window", FIELD(opt_amg_l0_window), window(int64_t(1) << 30), "0 (auto) or a multiple of 64 rows", kLayout,
     kDrops, E::kNone},
    {"amg_up_lanes", FIELD(opt_amg_up_lanes), list(0, 1, 2, 4), "0 (by width), 1, 2 or 4", false, kDrops,
     E::kLevelLanes},
    {"amg_coarse_rho_ppm", FIELD(opt_amg_coarse_rho_ppm), zero_or(100000, 100000000), "0 (Gershgorin) or 1e5 .. 1e8",
     kLayout, kDrops, E::kOmega},
    {"amg_a0_slot", FIELD(opt_amg_a0_slot), kBit, "0 or 1", kLayout, kDrops, E::kNone},
    {"sweep_piece", FIELD(opt_sweep_piece), range(1, kOptSweepPieceMax), "1..64", kLayout, kDrops, E::kNone},
    {"amg_fuse_setup", FIELD(opt_amg_fuse_setup), kBit, "0 or 1", false, kDrops, E::kNone},
    {"amg_theta_ppm", FIELD(opt_amg_theta_ppm), range(0, 1000000), "0..1000000", kLayout, kDrops, E::kNone},
    {"amg_cycle", FIELD(opt_amg_cycle), kBit, "0 (four steps per level) or 1 (compact)", false, kDrops, E::kCycle},
    {"dist_timeout_ms", SCALED(dist_timeout_s, 1000), kAny, "milliseconds", false, kDrops, E::kNone},
    {"amg_reuse", FIELD(opt_amg_reuse), kBit, "0 (rebuild per active set) or 1", false, kDrops, E::kReuse},
    {"amg_rebuild_pct", FIELD(opt_amg_rebuild_pct), range(100, 100000), "100 .. 100000", false, kDrops, E::kNone},
    {"amg_rebuild_rent", FIELD(opt_amg_rebuild_rent), range(0, 100000), "0 .. 100000", false, kDrops, E::kNone},
    {"amg_dist", FIELD(opt_amg_dist), range(-1, 1),
     "0 (block Jacobi over partitions), 1 (global hierarchy), -1 (faster)", false, kDrops, E::kDistAuto},
    {"amg_rep_rows", FIELD(opt_amg_rep_rows), range(0, INT64_MAX), ">= 0", false, kDrops, E::kGlobalPlan},
    {"amg_dist_cycle", FIELD(opt_amg_dist_cycle), kBit, "0 (four-step) or 1 (compact)", false, kDrops,
     E::kGlobalPlan},
    {"dist_sums", FIELD(opt_dist_sums), kBit, "1 (all-reduce) or 0 (send / receive pairs)", false, kDrops,
     E::kDistSums},
    {"combo_graph", FIELD(opt_combo_graph), kBit, "0 or 1", false, kDrops, E::kNone},
    {"graph_start", FIELD(opt_graph_start), kBit, "0 or 1", false, kDrops, E::kNone},
    {"step_graph", FIELD(opt_step_graph), kBit, "0 or 1", false, kDrops, E::kNone},
    {"batch_graph", FIELD(opt_batch_graph), kBit, "0 or 1", false, kDrops, E::kNone},
    {"setup_entry", FIELD(opt_setup_entry), kBit, "0 or 1", false, kDrops, E::kNone},
    {"spec_post", FIELD(opt_spec_post), kBit, "0 or 1", false, kDrops, E::kNone},
    {"asm_kernel", FIELD(opt_asm_kernel), range(0, 2),
     "0 (row gather), 1 (element colours), 2 (element pass + row pass)", false, kDrops, E::kNone},
    {"cc_tile", FIELD(opt_cc_tile), list(512, 1024, 2048, 4096), "512, 1024, 2048 or 4096", false, kDrops, E::kNone},
    {"part_slack_pct", SCALED(opt_part_slack, 100), range(0, 45), "0..45", kLayout, kDrops, E::kNone},
    {"keep_operator", FIELD(opt_keep_operator), kBit, "0 or 1", false, OptKeeps::kWhenSet, E::kNone},
    {"amg_close", FIELD(opt_amg_close), kBit, "0 or 1", false, kKeeps, E::kNone},
    {"amg_start", FIELD(opt_amg_start), kBit, "0 or 1", false, kKeeps, E::kNone},
    {"amg_lazy_px", FIELD(opt_amg_lazy_px), kBit, "0 or 1", false, kKeeps, E::kNone},
    {"amg_big_chunk", FIELD(opt_amg_big_chunk), range(2, kOptBigChunkMax), "2..63", false, kKeeps, E::kNone},
};
#undef FIELD
#undef SCALED

}  // namespace

int option_count() { return (int)(sizeof kOptions / sizeof kOptions[0]); }
const OptionDesc& option_at(int i) { return kOptions[i]; }

const OptionDesc* find_option(const char* name) {
  for (const OptionDesc& d : kOptions)
    if (std::strcmp(d.name, name) == 0) return &d;
  return nullptr;
}

bool option_legal(const OptionDesc& d, int64_t value) {
  const OptLegal& l = d.legal;
  switch (l.kind) {
    case OptLegal::kAny:
    case OptLegal::kFlag:
      return true;
    case OptLegal::kRange:
      return value >= l.v[0] && value <= l.v[1];
    case OptLegal::kZeroOrRange:
      return value == 0 || (value >= l.v[0] && value <= l.v[1]);
    case OptLegal::kWindow:
      return value >= 0 && value % 64 == 0 && value <= l.v[0];
    case OptLegal::kList:
      for (int i = 0; i < l.n; ++i)
        if (value == l.v[i]) return true;
      return false;
  }
  return false;
}

void option_store(const OptionDesc& d, Options& o, int64_t value) {
  d.store(o, d.legal.kind == OptLegal::kFlag ? (int64_t)(value != 0) : value);
}

}  // namespace mfea
