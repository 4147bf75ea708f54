// capi.hip — the C ABI of include/mfea.h: handle, device memory, the on-device
// step loop (assemble → RHS → PCG in hipGraph-captured chunks → reaction/stress),
// and the multi-partition driver (partition.hpp): one partition per GPU joined
// over RCCL (mfea_dist_init), or several partitions on one device exchanging
// through device copies (mfea_debug_set_parts; the same kernels and the same
// exchange schedule, used to test the partitioned solve on one GPU).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <deque>
#include <limits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "amg.hpp"
#include "amg_kernels.hpp"
#include "carve.hpp"
#include "kernels.hpp"
#include "mfea_debug.h"
#include "mfea.h"
#include "options.hpp"
#include "partition.hpp"
#include "records.hpp"
#include "run.hpp"
#include "symbolic.hpp"

using namespace mfea;

namespace {

thread_local std::string g_err;

// MFEA_BUILD_TIMES=1 (as amg_symbolic.cpp's build split): the host side of a
// new active set on stderr — failed-id tracking, plan build, upload, mask
struct HostLap {
  bool on = std::getenv("MFEA_BUILD_TIMES") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char* what, int64_t n = -1) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    if (n >= 0)
      std::fprintf(stderr, "  host %-26s %8.3f ms  (%lld)\n", what, std::chrono::duration<double, std::milli>(now - t).count(), (long long)n);
    else
      std::fprintf(stderr, "  host %-26s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPC(call)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(MFEA_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_));       \
  } while (0)

#define NCCLC(call)                                                                       \
  do {                                                                                    \
    ncclResult_t r_ = (call);                                                             \
    if (r_ != ncclSuccess)                                                                \
      return fail(MFEA_ECOMM, std::string(#call) + ": " + ncclGetErrorString(r_));        \
  } while (0)

#define RC(call)                  \
  do {                            \
    if (int rc_ = (call)) return rc_; \
  } while (0)

template <class T>
struct DevBuf {
  T* ptr = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    n = 0;
  }
  hipError_t alloc(size_t count) {
    if (count <= n && ptr) return hipSuccess;
    release();
    n = count;
    return hipMalloc(&ptr, std::max<size_t>(count, 1) * sizeof(T));
  }
};

}  // namespace

// One partition's operator, vectors and solver state on the handle's device.
// Single-GPU handles hold one partition covering the whole mesh.
struct Part {
  int rank = 0;   // partition index = rank in the partitioned solve
  Pattern P;      // local pattern (the whole mesh when not partitioned)
  PartPlan plan;  // partitioned only
  DevBuf<double> xyz_d, val, diag, x, r, p, q, dinv, stress, partials, red;
  DevBuf<double> cg_r1, cg_s0, cg_s1, cg_w0, cg_w1;  // CG-CG double buffers (r0 = r)
  DevBuf<double> cg_part;                            // CG-CG block partials, 2 parities; a third buffer:
                                                     // the closing check's (k_amg_rnorm)
  DevBuf<int32_t> slice_ptr, row_len, s_col, s_elem, e2n_d;
  DevBuf<uint8_t> active, code, elem_own;
  DevBuf<int32_t> fail_list;  // (owned) elements failed in the last post (any order)
  DevBuf<int32_t> event_of;   // mfea_event / mfea_run_events: the event that failed each element (-1: none)
  DevBuf<double> eps;         // the event scan's strains, for k_event_apply (option "event_scratch")
  DevBuf<int32_t> amg_inv;    // Pattern row → level-0 row (k_amg_start), for the plan below
  int64_t amg_inv_gen = -1;
  const int32_t* amg_inv_row0 = nullptr;
  DevBuf<unsigned> fail_cnt;
  DevBuf<unsigned> tickets;
  // mfea_get_energy, allocated at its first use on this build: a caller's U in
  // row order, a caller's mask, the rows asked for (up to four of E doubles)
  // with the two totals behind them, and the reduction's own partials and
  // ticket set (no captured graph and no enqueued post holds either)
  DevBuf<double> en_u, en_out, en_part;
  DevBuf<uint8_t> en_act;
  DevBuf<unsigned> en_tix;
  // mfea_set_grip_field: the field's vectors of the known rows in row order
  // (bc_form.hpp GripField; at least 3 doubles), uploaded by the setter and at
  // each build; mfea_get_grip_work's outputs (sums[0..2] of a band, the value)
  DevBuf<double> grip_d, gw_red;
  // mfea_set_node_loads: the loads of the free rows in row order (bc_form.hpp
  // NodeLoad; at least 3 doubles), uploaded by the setter and at each build;
  // the floating mask of the free rows in row order (launch_floating, label
  // NULL) with the act_gen it reflects (−1: none yet) — recomputed only while
  // loads are set; the form the kernels take; mfea_get_load_work's output
  DevBuf<double> ld_f, lw_red;
  DevBuf<uint8_t> ld_mask;
  int64_t ld_mask_gen = -1;
  NodeLoad ld{};
  // wave-local lane operator (ell.hip); ell_ok = false → SELL kernel
  Ell L;
  bool ell_ok = false;
  bool ell_hc = false;  // compact halo records (ell_op)
  DevBuf<uint32_t> e_code;
  DevBuf<int32_t> e_partner, e_lane_row, e_src_pos, e_nbr_lane, e_hbase;
  DevBuf<uint64_t> e_hmask;
  DevBuf<double> e_f;  // all lane-operator doubles, carved by ell_op / ell_vecs
  DevBuf<Slot> slots;
  DevBuf<SolveState> state, state_mirror;
  SolveState* mirror = nullptr;  // where k_cg_advance publishes the final state
  int64_t G = 0;                 // slots·64
  // partitioned solve: exchange buffers
  DevBuf<double> xrec;  // xs[2] | xr[2] | mr
  DevBuf<double> gbuf;  // gall[2] | gsend | gred
  DevBuf<double> xh;    // displacement halo: send | recv
  DevBuf<int32_t> xsend_rows, xrecv_rows;
  DistVecs dv{};
  double* gred = nullptr;  // [64][4] gathered scalars (RHS norms, reaction, #active)
  double* xh_send = nullptr;
  double* xh_recv = nullptr;
  // SA-AMG preconditioner (amg.hpp): symbolic plan for the active set amg_key
  AmgPlan amg;
  AmgCollapse amg_coll;  // the compact cycle below level kc as one operator (amg_collapse.cpp)
  AmgMerge amg_mplan;    // levels 0 and 1 merged around the collapsed cycle (amg.hpp AmgMerge)
  AmgMergeD amg_mg;
  float* amg_x2 = nullptr;  // level 2's own x / e (the merged cycle points them into amg_mg.B)
  float* amg_e2 = nullptr;
  bool amg_ok = false;
  std::vector<uint8_t> amg_key;
  int64_t amg_gen = 0;               // bumped on every rebuild (captured graphs hold its pointers)
  int64_t fmask_gen = 0;             // bumped on every enqueue_fmask (the setup reads amg_fmask)
  // what the hierarchy's values were last formed from (option keep_operator):
  // the setup launches' arguments (key), K, the plan, the floating mask; ok
  // only once the solve behind that setup ended with status 0.  ω: every
  // change goes through apply_coarse_omega, which clears ok.
  struct {
    bool ok = false;
    uint64_t key = 0;
    int64_t op_gen = -1, amg_gen = -1, fmask_gen = -1;
  } kept;
  int amg_last_iters = 0;            // iterations of the last converged GAMG solve (chunk plan)
  // a hierarchy kept over element failures (option amg_reuse): the activity
  // its floating-row mask reflects, the iterations of its first solve, and
  // whether a later solve degraded enough to rebuild
  DevBuf<uint8_t> amg_fmask;         // level-0 rows of floating pieces (kernels.hpp launch_floating)
  const int32_t* amg_row0_inv = nullptr;  // level-0 label of every free row (carved from amg_i)
  DevBuf<int32_t> cc_parent;         // launch_floating's scratch: component links, anchored roots
  DevBuf<uint8_t> cc_anch;
  // element colouring for the element-centric assembly (option asm_kernel 1),
  // built at first use: ec_state 0 not built, 1 usable, -1 not colourable
  ElemColour ec;
  int ec_state = 0;
  DevBuf<int32_t> ec_entry, ec_pos;
  // the plan's key covers the current activity: act_sub_gen when it was
  // built or last compared (failures only ever shrink the set, so it holds
  // until the activity is set explicitly), and its element count
  int64_t amg_sub_gen = -1;
  int64_t amg_key_count = 0;
  int amg_build_iters = -1;
  // the kept hierarchy's rent (option amg_rebuild_rent): the host time its
  // build took, and the time its solves have spent since on iterations above
  // amg_build_iters — a rebuild is bought once the rent paid reaches its price
  double amg_build_s = 0.0;
  double amg_excess_s = 0.0;
  bool amg_stale = false;
  bool amg_reused = false;           // the last ensure_amg kept a hierarchy built for another set
  int64_t amg_seen_gen = -1;         // act_gen at which the plan / mask last matched the activity
  DevBuf<int32_t> amg_i;             // every index array of the plan, carved
  DevBuf<double> amg_d;              // every f64 value / vector array, carved
  DevBuf<float> amg_f;               // the f32 V-cycle copies and vectors, carved
  std::vector<AmgLevD> amg_lev;      // device views
  DevBuf<AmgLevD> amg_levd;          // … and their device copy (the setup tail reads it)
  bool amg_om_own = false;           // the hierarchy is this partition's own (not a split global one)
  bool amg_om_spatial = false;       // ... on Z-ordered labels (level 0's one-pass setup)
  int amg_tail = 0;                  // first level of the single-workgroup tail (0: none)
  int amg_first = 1;                 // first level the four-step tail may start at (not split)
  AmgCg amg_cg;
  // the V-cycle outputs u of a chunk, one slot per update (option amg_lazy_px,
  // amg_kernels.hpp AmgPx); null: partitioned or a one-level plan
  float* amg_uh = nullptr;
  int64_t amg_uh_stride = 0;
  // level 0's block halo plan (option amg_fuse_l0, amg.hpp AmgFusePlan): the
  // last up sweep and w = A u in one launch (amg.hip k_amg_up_w) while on
  AmgFusePlan amg_fplan;
  AmgFuseD amg_fuse;
  // the plan's preconditioner kind: MFEA_PC_GAMG (the hierarchy) or a
  // one-level plan with multicolour sweeps (MFEA_PC_SOR / MFEA_PC_ICC, sweep.hip)
  int amg_kind = MFEA_PC_GAMG;
  SweepPlan sweep;
  SweepD swd;
  DevBuf<int32_t> sw_i;   // the plan's entry arrays and cross lists
  DevBuf<float> sw_f;     // pv | D̃⁻¹ | lov | upv (formed per solve)
  DevBuf<double> sw_y;    // the sweeps' iterate
  const int32_t* amg_a0_ptr = nullptr;
  const int32_t* amg_a0_a = nullptr;
  // partitioned GAMG (amg.hpp AmgHalo): ghost couplings and the u halo
  AmgHalo amg_halo;
  AmgDist amg_dist;
  DevBuf<int32_t> amg_hi;  // send_rows | gptr | gslot | grecv
  DevBuf<double> amg_hd;   // usend | urecv
  // distributed GAMG over the global hierarchy (mfea_handle::gamg): this
  // partition's rows and exchange plans (amg.hpp AmgRank), the plans' item
  // lists on the device and the staging buffers of one exchange
  AmgRank amg_rank;
  PosList g_a0;                 // its level-0 lists over this partition's pattern
  std::vector<int32_t> g_row0;
  int dev_plan = -1;            // which plan the device arrays hold: 0 its own (pt.amg), 1 the global one
  struct XDev {
    const XPlan* x = nullptr;
    const int32_t* s = nullptr;  // sidx
    const int32_t* r = nullptr;  // ridx
  };
  std::vector<XDev> xd_a, xd_r, xd_p, xd_sp, xd_sap;
  XDev xd_g, xd_sg;
  XDev xd_c, xd_spt, xd_sd;  // the compact cycle split at level 0 (AmgRank::compact)
  DevBuf<int32_t> amg_xi;
  DevBuf<double> amg_xs, amg_xr;
  // mfea_run (run.hpp): iperm of this build's pattern and the two staging
  // slabs, allocated at the first run after a (re)build
  DevBuf<int32_t> iperm_d;
  DevBuf<uint8_t> rec_slab[2];
  bool rec_ok = false;
};

// What the assembly and post kernels take their material from: the scalars by
// value and the generation of the per-element properties (their device
// pointers and the uniform / per-element kernel choice).  Compared and hashed
// wherever K or a captured graph remembers what it was formed with.
struct MatKey {
  Material mat{};
  int64_t props_gen = 0;
  bool operator==(const MatKey& o) const {
    return std::memcmp(&mat, &o.mat, sizeof mat) == 0 && props_gen == o.props_gen;
  }
  bool operator!=(const MatKey& o) const { return !(*this == o); }
};

// (the tuning options and their defaults: Options, options.hpp)
struct mfea_handle : Options {
  int device = 0;
  hipStream_t stream = nullptr;
  double E = 2500.0, A = 0.0, I = 0.0;
  Material mat{};
  // mfea_set_element_props (one partition): the columns the caller gave, in
  // element order (empty: the handle's scalar / the call's max_strain), and
  // what the kernels read — the interleaved (EA_e, EI12_e) pairs when any of
  // E, A, I is an array, E_e, max_strain_e.  props_gen: bumped by every change
  // of them (monotonic; MatKey).
  std::vector<double> pe_E, pe_A, pe_I, pe_S;
  std::vector<double> pe_sec;  // host copy of the pairs (the AMG strength estimate)
  DevBuf<double> pe_sec_d, pe_E_d, pe_S_d;
  int64_t props_gen = 0;
  MatKey mat_key() const { return MatKey{mat, props_gen}; }
  bool has_props() const { return !pe_E.empty() || !pe_A.empty() || !pe_I.empty() || !pe_S.empty(); }
  const double2* sec_d() const { return pe_sec.empty() ? nullptr : reinterpret_cast<const double2*>(pe_sec_d.ptr); }
  const double* Ee_d() const { return pe_E.empty() ? nullptr : pe_E_d.ptr; }
  const double* strength_d() const { return pe_S.empty() ? nullptr : pe_S_d.ptr; }
  // What is prescribed on the boundary and the free nodes (one partition),
  // handle state as the material is; nothing of K or the hierarchies depends
  // on it.  form() is what every launcher is told (bc_form.hpp BcForm).
  struct Loading {
    // mfea_set_grip_motion: the directions of the grip motion.  The tensile
    // test's pair takes the kernels as they were (the GripY instantiations);
    // any other the GripVec ones.
    GripVec grip{{0.0, 1.0, 0.0}, {0.0, 1.0, 0.0}};
    // mfea_set_grip_field: a vector per node, original node order, host copy.
    // While set it takes the place of the two directions everywhere (they are
    // kept, and read nowhere): the GripField kernels.
    NodeVectors field;
    // mfea_set_node_loads: a force vector per node, original node order, host
    // copy; the mode; dy_top of the last solve (mfea_get_load_work)
    NodeVectors loads;
    int32_t load_mode = MFEA_LOAD_DEAD;
    double load_dy_top = 0.0;
    bool grip_default() const {
      return grip.top[0] == 0.0 && grip.top[1] == 1.0 && grip.top[2] == 0.0 && grip.bot[0] == 0.0 &&
             grip.bot[1] == 1.0 && grip.bot[2] == 0.0;
    }
    bool grip_z() const { return field.set ? field.z() : grip.top[2] != 0.0 || grip.bot[2] != 0.0; }
    bool load_z() const { return loads.z(); }
    // (the field's and the loads' rows of pt: upload_rows, at the setters and at each build)
    BcForm form(const Part& pt) const {
      return BcForm{grip_default() ? nullptr : &grip, field.set ? pt.grip_d.ptr : nullptr,
                    loads.set ? &pt.ld : nullptr};
    }
  } bc;
  // host-side mesh/BC (original order)
  int64_t N = 0, Ecount = 0;
  std::vector<double> xyz;
  std::vector<int64_t> e2n;
  uint32_t mesh_flags = 0;
  bool planar = false;  // every z == 0 (the whole mesh)
  std::vector<int64_t> top, bot;
  int64_t n_free_global = 0;
  bool has_mesh = false, dirty = true;
  bool assembled = false;  // the operator holds an assembly since the last (re)build
  std::vector<uint8_t> active_host;  // pending upload, original element order (empty = none)
  std::vector<std::unique_ptr<Part>> parts;
  // partitioning: nparts partitions on this device (world == 1), or this
  // process's partition `rank` of `world` (RCCL)
  int nparts = 1, axis = -1;
  int world = 1, rank = 0;
  ncclComm_t comm = nullptr;
  SolveState* h_state = nullptr;       // pinned, 2 entries
  SolveState* d_host_state = nullptr;  // device view of h_state (mapped)
  double* h_red = nullptr;             // pinned
  // graph cache (single partition)
  hipGraphExec_t graph = nullptr;
  int graph_chunk = 0, graph_precond = -1, graph_ell = -1;
  hipGraphExec_t graph_big = nullptr;  // GAMG: the planned batch's long chunks
  int graph_big_chunk = 0, graph_big_ell = -1;
  // GAMG: the planned batch's remainder at its exact length, one graph per
  // length (the expected count moves between solves: failures, rebuilds)
  static constexpr int kRemGraphs = 64;
  hipGraphExec_t graph_rem[kRemGraphs] = {};
  int graph_rem_ell = -1;
  // mfea_step (option "batch_graph"): the planned batch as ONE graph of its
  // exact length with the finish and the post kernels behind it, one graph
  // per length, keyed by the plan and the failure strain
  hipGraphExec_t graph_batch[kRemGraphs] = {};
  // ... and (option "combo_graph") behind the numeric setup in the setup's
  // graph: one graph launch per step, one cached graph per batch length
  // Both in two forms, cached side by side — [0] with the numeric setup, [1]
  // without it (option keep_operator: a kept setup, or one launched as its
  // own graph in front, solve_amg) — so a run that goes from kept steps to a
  // failure step and back replays, never recaptures
  hipGraphExec_t graph_combo[2][kRemGraphs] = {};
  uint64_t graph_combo_key[2][kRemGraphs] = {};
  int graph_batch_ell = -1;
  double graph_batch_strain = 0.0;
  // GAMG: the numeric setup's launches (≈ 30) as one graph, keyed by a hash
  // of every argument they take (the level views, the level-0 operator, reg)
  hipGraphExec_t graph_setup[2] = {};  // ([1]: the head / entry launches alone)
  uint64_t graph_setup_key[2] = {};
  hipEvent_t ev[6] = {};
  hipEvent_t ev_setup = nullptr;
  bool ev_setup_used = false;  // the last solve recorded ev_setup (GAMG)
  bool in_step = false;        // mfea_step: the solve's end is waited for by post
  // mfea_step's assembly also formed the GAMG solves' RHS for these grip
  // displacements (AsmRhs); the next solve_amg uses it instead of k_amg_rhs
  bool rhs_fused = false;
  double rhs_dy[2] = {0.0, 0.0};
  int64_t op_gen = 0;  // bumped by every launch that writes val / diag
  struct {
    bool ok = false;
    int64_t act_gen = -1;
    MatKey mat{};
    int asm_kernel = -1;
  } k_from;
  int last_precond = -1;          // the last solve's preconditioner kind
  int64_t op_kept_steps = 0;      // read-only option: steps that skipped the assembly
  int64_t amg_setup_kept = 0;     // read-only option: solves that skipped the numeric setup
  int64_t amg_close_hits = 0;     // read-only option: solves that ended at the closing check
  int amg_last_cycles = 0;        // read-only option: preconditioner applications the last GAMG solve queued
  int64_t amg_start_fused = 0;    // read-only option: solves that started with k_amg_start
  int64_t amg_px_replays = 0;     // read-only option: replay launches queued by the solves
  bool setup_skipped = false;     // the last solve did (phase times: t_setup_ms = 0)
  MatKey graph_batch_mat{};       // the material / properties graph_batch's post kernels were captured with
  bool asm_pending = false;  // mfea_step deferred its assembly to solve_amg
  DevBuf<double> d_dy;
  bool spec_on = false;
  bool spec_used = false;  // one speculative post per step: behind the planned batch only
  bool spec_launched = false;
  double spec_strain = 0.0;
  // mfea_event / mfea_run_events: the post of this step is the event pair
  // (k_event_scan, k_event_apply; events.hip) with these parameters.  It rides
  // where the post rides behind an eagerly launched batch (spec_post, undone
  // by k_event_unfail); the batch graph holds the plain post only, so an event
  // step does not take it.
  bool ev_on = false;
  double ev_strain = 0.0, ev_tie = 0.0, ev_lam_max = 0.0;
  int32_t ev_index = 0;
  hipEvent_t poll[2] = {};
  int64_t n_active = 0;
  bool act_all = false;  // every element is active on the device (set_active(NULL), no failure since)
  // host view of the element activity (single partition; keys the AMG plan):
  // exact after set_active / a build, stale once a post kernel deactivated
  // elements (then downloaded on demand)
  std::vector<uint8_t> act_host;
  bool act_host_ok = false;
  int64_t act_count = 0;
  bool amg_safe_omega = false;  // read-only option: a solve failed at amg_coarse_rho_ppm; ω is the safe value
  // distributed GAMG (partitioned handles, option "amg_dist" 1): the whole
  // mesh's pattern and node owners (built with the partitions), and ONE
  // global hierarchy for the current global element activity
  Pattern gpat;
  std::vector<int32_t> gowner;
  AmgPlan gamg;
  std::vector<uint8_t> gamg_key;  // the global activity gamg was built for
  // partitioned: the global element activity on the host, exact at act_gen
  // gkey_gen (set by mfea_set_active, moved by the failed-element ids every
  // post exchanges — global_active)
  std::vector<uint8_t> gkey;
  int64_t gkey_gen = -1;
  DevBuf<int32_t> gfail;  // RCCL: failed-id all-gather buffers
  bool gamg_ok = false;
  int64_t gamg_gen = 0;       // bumped on every upload (captured graphs hold its pointers)
  int64_t gamg_plan_gen = 0;  // bumped on every host rebuild (a new active set)
  int64_t act_gen = 1;        // bumped whenever the element activity may have changed
  int64_t act_sub_gen = 1;    // bumped when it changed other than by failures (set_active, a rebuild)
  int64_t gamg_act_gen = 0;   // act_gen the hierarchy was built for
  DevBuf<uint8_t> gact;       // RCCL: the global activity, max-all-reduced
  DevBuf<double> gtime;       // RCCL: a host time, max-all-reduced (amg_dist -1's choice)
  // option "amg_dist" -1: per active set (gamg_plan_gen), the first GAMG
  // solve runs the global hierarchy, the next block Jacobi; the faster
  // (host-timed, plan builds excluded) serves the set's further solves
  struct {
    int64_t gen = -1;
    int choice = -1;
    double t[2] = {-1.0, -1.0};
  } amg_auto;
  // mfea_run: the copy stream, per staging slab a "rows gathered" event (the
  // handle's stream) and a "slab free" event (the copy stream), and the two
  // pinned host slabs of the path without registered record arrays
  hipStream_t run_copy = nullptr;
  hipEvent_t run_ready[2] = {}, run_free[2] = {};
  uint8_t* run_pin[2] = {};
  size_t run_pin_bytes = 0;
  int run_direct = 0;            // read-only option "run_direct": the last run copied straight into them
  // generic CSR path scratch
  DevBuf<int64_t> c_indptr;
  DevBuf<int32_t> c_indices;
  DevBuf<double> c_data, c_kval, c_x, c_r, c_p, c_q, c_dinv;
  DevBuf<uint8_t> c_known;
};

namespace {

constexpr int kMaxChunk = 64;

// lane-operator doubles per lane: V 18, D 6, x 3, p 3, r/s/w × 2 18, M 6; plus per
// compact halo record (ell_vecs): h × 2 18, hM 6
constexpr int64_t kEllDoubles = 18 + 6 + 3 + 3 + 18 + 6 + 18 + 6;
static_assert(kEllNone == kSrcNone && kEllHalo == kSrcHalo, "slot source codes");
static_assert(kGhost == 3, "k_cg_rhs treats code 3 as a ghost free row");
constexpr int kTicketSets = 16;
constexpr int64_t kRecMax = 9, kMMax = 6;  // record / M widths at nd = 3, block Jacobi

Part& part0(mfea_handle* h) { return *h->parts[0]; }
bool partitioned(const mfea_handle* h) { return h->parts.size() > 1 || h->world > 1; }
int nranks(const mfea_handle* h) { return h->world > 1 ? h->world : (int)h->parts.size(); }
// a level's copies of the lane options
void set_level_lanes(const Options& o, AmgLevD& d) {
  d.rlanes = o.opt_amg_rlanes;
  d.dsplit = o.opt_amg_down_split;
  d.vlanes = o.opt_amg_v_lanes;
  d.small_lanes = o.opt_amg_small_lanes;
  d.alanes = o.opt_amg_alanes;
  d.tail_lds = o.opt_amg_tail_lds;
  d.ulanes = o.opt_amg_up_lanes;
}

// option keep_operator: forget what K and the hierarchies' values were formed
// from — the next step assembles, the next GAMG solve sets up
void drop_kept_setup(mfea_handle* h) {
  for (auto& pp : h->parts) pp->kept.ok = false;
}
void drop_kept(mfea_handle* h) {
  h->k_from.ok = false;
  drop_kept_setup(h);
}
// The per-element properties changed (or went): K, the hierarchies' values and
// every captured graph that holds a property pointer or a kernel's uniform /
// per-element form are the old ones' (MatKey) — the symbolic hierarchy stays,
// the active set did not move
void props_changed(mfea_handle* h) {
  ++h->props_gen;
  ++h->op_gen;
  drop_kept(h);
}
void clear_props(mfea_handle* h) {
  if (!h->has_props()) return;
  h->pe_E.clear();
  h->pe_A.clear();
  h->pe_I.clear();
  h->pe_S.clear();
  h->pe_sec.clear();
  props_changed(h);
}
// K (val / diag) is what an assembly would write now
bool k_current(const mfea_handle* h) {
  return h->opt_keep_operator && h->assembled && h->k_from.ok && h->k_from.act_gen == h->act_gen &&
         h->k_from.mat == h->mat_key() && h->k_from.asm_kernel == h->opt_asm_kernel;
}
// ... recorded by every launch that writes them
void k_written(mfea_handle* h) {
  ++h->op_gen;
  h->k_from.ok = true;
  h->k_from.act_gen = h->act_gen;
  h->k_from.mat = h->mat_key();
  h->k_from.asm_kernel = h->opt_asm_kernel;
}

// ticket set k (one per reducing kernel kind; see device_util.hpp layout)
unsigned* tix(Part& pt, int k) { return pt.tickets.ptr + (size_t)k * kTicketStride; }
// Host-facing copies and fills on the handle's stream, waited for.  The
// stream is non-blocking: a null-stream hipMemcpy / hipMemset is not ordered
// with it, so a fill of the activity could still be landing while the next
// assembly read it (an intermittent breakdown after set_active(NULL), a
// K assembled from a mix of the old and the new activity).
// The lifetime rule of every upload here: the host source of an asynchronous
// copy lives until the stream sync that follows it — a member, or a local of
// the frame that syncs, never of an inner block.
hipError_t hmemcpy(mfea_handle* h, void* dst, const void* src, size_t n, hipMemcpyKind k) {
  const hipError_t e = hipMemcpyAsync(dst, src, n, k, h->stream);
  return e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
}
// ... not waited for (nothing to copy: no call)
hipError_t h2d_async(mfea_handle* h, void* dst, const void* src, size_t bytes) {
  return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
}
// The index arrays carved from one allocation (carve.hpp).  stage_begin: st
// has counted them — buf gets that size and the fill pass starts.
// stage_flush: every array the fill listed goes up, straight from its vector,
// and the stream is waited for HERE, error or not: the sources (the plan's
// vectors, locals of the uploader's frame) are free when it returns.
int stage_begin(DevBuf<int32_t>& buf, IndexStage& st) {
  HIPC(buf.alloc(std::max<size_t>(st.size(), 1)));
  st.begin_fill();
  return 0;
}
int stage_flush(mfea_handle* h, DevBuf<int32_t>& buf, const IndexStage& st) {
  if (st.offset() != st.size() || st.size() > buf.n)
    return fail(MFEA_EINVAL, "internal: a plan upload's sizing and fill passes differ");
  hipError_t e = hipSuccess;
  for (const IndexStage::Item& it : st.items())
    if (e == hipSuccess) e = h2d_async(h, buf.ptr + it.at, it.v->data(), it.v->size() * sizeof(int32_t));
  const hipError_t es = hipStreamSynchronize(h->stream);
  HIPC(e != hipSuccess ? e : es);
  return 0;
}
// Waits for what earlier calls left on the stream (assemblies, activity
// updates, solves on a current plan) before a plan upload, so that their fault
// is reported as theirs and not as the upload's first checked call.
int drain_before_upload(mfea_handle* h, const char* what) {
  const hipError_t e = hipStreamSynchronize(h->stream);
  return e == hipSuccess ? 0 : fail(MFEA_EDEVICE, std::string("before ") + what + ": " + hipGetErrorString(e));
}
hipError_t hmemset(mfea_handle* h, void* dst, int v, size_t n) {
  const hipError_t e = hipMemsetAsync(dst, v, n, h->stream);
  return e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
}

// The device form of the per-element properties from the host columns and the
// handle's scalars: EA_e = E_e*A_e and EI12_e = (12.0*E_e)*I_e, the expressions
// and rounding of mfea_set_material.  The stream is drained first (a kernel of
// an earlier call may still read the arrays) and after.
int upload_props(mfea_handle* h) {
  const int64_t n = h->Ecount;
  props_changed(h);
  h->pe_sec.clear();
  if (!h->has_props() || n <= 0) return 0;
  HIPC(hipStreamSynchronize(h->stream));
  if (!h->pe_E.empty() || !h->pe_A.empty() || !h->pe_I.empty()) {
    h->pe_sec.resize(2 * n);
    for (int64_t e = 0; e < n; ++e) {
      const double E = h->pe_E.empty() ? h->E : h->pe_E[e];
      const double A = h->pe_A.empty() ? h->A : h->pe_A[e];
      const double I = h->pe_I.empty() ? h->I : h->pe_I[e];
      h->pe_sec[2 * e] = E * A;
      h->pe_sec[2 * e + 1] = (12.0 * E) * I;
    }
    HIPC(h->pe_sec_d.alloc(2 * n));
    HIPC(hmemcpy(h, h->pe_sec_d.ptr, h->pe_sec.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!h->pe_E.empty()) {
    HIPC(h->pe_E_d.alloc(n));
    HIPC(hmemcpy(h, h->pe_E_d.ptr, h->pe_E.data(), n * sizeof(double), hipMemcpyHostToDevice));
  }
  if (!h->pe_S.empty()) {
    HIPC(h->pe_S_d.alloc(n));
    HIPC(hmemcpy(h, h->pe_S_d.ptr, h->pe_S.data(), n * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
}

// Rows [row0, row0 + n) of a per-node array gathered into Pattern row order
// (row row0 + r at 3r; at least 3 doubles) and uploaded into dst; waited for,
// before and after.
static int upload_rows(mfea_handle* h, const Pattern& P, const std::vector<double>& nodes, int64_t row0, int64_t n,
                       DevBuf<double>& dst) {
  std::vector<double> rows((size_t)3 * std::max<int64_t>(n, 1), 0.0);
  for (int64_t r = 0; r < n; ++r)
    for (int c = 0; c < 3; ++c) rows[3 * r + c] = nodes[3 * (size_t)P.perm[row0 + r] + c];
  HIPC(hipStreamSynchronize(h->stream));
  HIPC(dst.alloc(rows.size()));
  HIPC(hmemcpy(h, dst.ptr, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
// The grip field's vectors of the known rows (row j at 3·(j − n_free)).
int upload_field(mfea_handle* h, Part& pt) {
  return upload_rows(h, pt.P, h->bc.field.v, pt.P.n_free, pt.P.n_nodes - pt.P.n_free, pt.grip_d);
}
// The nodal loads of the free rows.  The floating mask of this build starts as
// zeros and counts as not computed (ensure_load_mask); it depends on the
// activity alone, so other loads on the same build keep it.
int upload_loads(mfea_handle* h, Part& pt) {
  const Pattern& P = pt.P;
  RC(upload_rows(h, P, h->bc.loads.v, 0, P.n_free, pt.ld_f));
  if (!pt.ld_mask.ptr) {
    HIPC(pt.ld_mask.alloc(std::max<int64_t>(P.n_free, 1)));
    HIPC(hmemset(h, pt.ld_mask.ptr, 0, std::max<int64_t>(P.n_free, 1)));
    pt.ld_mask_gen = -1;
  }
  pt.ld = NodeLoad{pt.ld_f.ptr, pt.ld_mask.ptr, h->bc.load_mode == MFEA_LOAD_PROPORTIONAL ? 1 : 0};
  return 0;
}

// The floating mask the load kernels read, of the device's current activity:
// recomputed (launch_floating in row order, four launches on the stream, no
// wait) when the activity has moved since it was formed — only while loads
// are set.  Called in front of every assembly and step, outside any capture,
// so the mask is that of the activity the step's K is assembled from.
int ensure_load_mask(mfea_handle* h) {
  if (!h->bc.loads.set || h->parts.size() != 1) return 0;
  Part& pt = *h->parts[0];
  const Pattern& P = pt.P;
  if (pt.ld_mask_gen == h->act_gen || P.n_free == 0) return 0;
  HIPC(pt.cc_parent.alloc(std::max<int64_t>(P.n_nodes, 1)));
  HIPC(pt.cc_anch.alloc(std::max<int64_t>(P.n_nodes, 1)));
  launch_floating(h->stream, P.n_nodes, P.n_free, P.n_nodes - P.n_ghost, pt.slice_ptr.ptr, pt.row_len.ptr,
                  pt.s_col.ptr, pt.s_elem.ptr, pt.active.ptr, pt.cc_parent.ptr, pt.cc_anch.ptr, nullptr,
                  pt.ld_mask.ptr, h->opt_cc_tile);
  HIPC(hipGetLastError());
  pt.ld_mask_gen = h->act_gen;
  return 0;
}

double* cg_part_buf(Part& pt, int par) { return pt.cg_part.ptr + (size_t)par * 4 * kCgMaxPartials; }

void destroy_graph(mfea_handle* h) {
  if (h->graph) (void)hipGraphExecDestroy(h->graph);
  if (h->graph_big) (void)hipGraphExecDestroy(h->graph_big);
  h->graph_big = nullptr;
  h->graph_big_chunk = 0;
  h->graph_big_ell = -1;
  for (auto& g : h->graph_rem) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
  h->graph_rem_ell = -1;
  for (auto& g : h->graph_batch) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
  h->graph_batch_ell = -1;
  // (not the combined graphs: one may be in flight when the solve recaptures
  // its chunk graphs; their keys replace them, mfea_destroy frees them)
  h->graph = nullptr;
  h->graph_chunk = 0;
  h->graph_precond = -1;
  h->graph_ell = -1;
}

int set_device(mfea_handle* h) {
  HIPC(hipSetDevice(h->device));
  return 0;
}

// Row ordering of the free nodes: DFS by default (option "order": -1 DFS,
// 0 natural, > 1 degree sort inside windows of that many rows).
int order_mode(const mfea_handle* h) { return h->opt_order; }

// planar meshes run with 2 DOFs per node (option "lane_dof" 3 forces 3, and
// so does a grip motion with a z component: the solution leaves the plane);
// decided on the whole mesh so every partition exchanges records of one width
// (grip_z: of the field's rows while a grip field is set; load_z: a nodal load
// with a z entry takes the solution out of the plane as well)
int lane_dofs(const mfea_handle* h) {
  return (h->planar && h->opt_lane_dof != 3 && !h->bc.grip_z() && !h->bc.load_z()) ? 2 : 3;
}

// Waits for an event.  Partitioned over RCCL: polls with a deadline and the
// communicator's error state, so a lost peer ends the call instead of hanging.
int wait_event(mfea_handle* h, hipEvent_t ev) {
  if (h->world <= 1 || !h->comm) {
    HIPC(hipEventSynchronize(ev));
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return fail(MFEA_EDEVICE, std::string("hipEventQuery: ") + hipGetErrorString(e));
    ncclResult_t ar = ncclSuccess;
    if (ncclCommGetAsyncError(h->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress) {
      (void)ncclCommAbort(h->comm);
      h->comm = nullptr;
      return fail(MFEA_ECOMM, std::string("RCCL: ") + ncclGetErrorString(ar));
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (dt > h->dist_timeout_s) {
      (void)ncclCommAbort(h->comm);
      h->comm = nullptr;
      return fail(MFEA_ECOMM, "RCCL: no progress before the deadline (peer lost?)");
    }
    // spin for the first 200 µs (a converged chunk or a step's end is
    // usually that close), then poll every 20 µs
    if (dt > 200e-6) std::this_thread::sleep_for(std::chrono::microseconds(20));
    else std::this_thread::yield();
  }
}

// a phase boundary for mfea_stats (only with option phase_times)
int phase_event(mfea_handle* h, hipEvent_t ev, hipStream_t s) {
  if (h->opt_phase_times) HIPC(hipEventRecord(ev, s));
  return 0;
}

int sync_stream(mfea_handle* h) {
  HIPC(hipEventRecord(h->ev[5], h->stream));
  return wait_event(h, h->ev[5]);
}

// ---------------------------------------------------------------------------
// Build one partition: symbolic pattern + lanes (host), allocate and upload.
// ---------------------------------------------------------------------------
int upload_part(mfea_handle* h, Part& pt, bool dm) {
  const Pattern& P = pt.P;
  const int64_t N = P.n_nodes, E = P.n_elems;
  pt.G = P.n_slots() * kSlice;
  const int64_t maxg = std::max<int64_t>({grid_rows(N), grid_rows(E), 2048, 1});
  HIPC(pt.xyz_d.alloc(3 * N));
  HIPC(pt.val.alloc(6 * pt.G));
  HIPC(pt.diag.alloc(6 * N));
  HIPC(pt.x.alloc(3 * N));
  HIPC(pt.r.alloc(3 * N));
  HIPC(pt.p.alloc(3 * N));
  HIPC(pt.q.alloc(3 * N));
  HIPC(pt.cg_r1.alloc(3 * N));
  HIPC(pt.cg_s0.alloc(3 * N));
  HIPC(pt.cg_s1.alloc(3 * N));
  HIPC(pt.cg_w0.alloc(3 * N));
  HIPC(pt.cg_w1.alloc(3 * N));
  HIPC(pt.cg_part.alloc(3 * 4 * kCgMaxPartials));
  HIPC(pt.dinv.alloc(6 * N));
  HIPC(pt.stress.alloc(E));
  HIPC(pt.partials.alloc(5 * (maxg + 16)));  // (the widest user: the event scan with three reaction sums)
  HIPC(pt.red.alloc(16));
  HIPC(pt.slice_ptr.alloc(P.slice_ptr.size()));
  HIPC(pt.row_len.alloc(N));
  HIPC(pt.s_col.alloc(pt.G));
  HIPC(pt.s_elem.alloc(pt.G));
  HIPC(pt.e2n_d.alloc(2 * E));
  HIPC(pt.active.alloc(E));
  HIPC(pt.code.alloc(N));
  HIPC(pt.tickets.alloc(kTicketSets * kTicketStride));
  HIPC(pt.slots.alloc(kMaxChunk + 2));
  HIPC(pt.state.alloc(1));
  hipStream_t s = h->stream;
  // the host sources built here: alive until the sync at the end (hmemcpy's rule)
  std::vector<uint8_t> act;
  std::vector<uint32_t> code;
  std::vector<int32_t> push, rs, rr;
  HIPC(h2d_async(h, pt.xyz_d.ptr, P.xyz_perm.data(), 3 * N * sizeof(double)));
  HIPC(h2d_async(h, pt.slice_ptr.ptr, P.slice_ptr.data(), P.slice_ptr.size() * sizeof(int32_t)));
  HIPC(h2d_async(h, pt.row_len.ptr, P.row_len.data(), N * sizeof(int32_t)));
  HIPC(h2d_async(h, pt.s_col.ptr, P.s_col.data(), pt.G * sizeof(int32_t)));
  HIPC(h2d_async(h, pt.s_elem.ptr, P.s_elem.data(), pt.G * sizeof(int32_t)));
  HIPC(h2d_async(h, pt.e2n_d.ptr, P.e2n_perm.data(), 2 * E * sizeof(int32_t)));
  HIPC(h2d_async(h, pt.code.ptr, P.code.data(), N * sizeof(uint8_t)));
  HIPC(hipMemsetAsync(pt.tickets.ptr, 0, kTicketSets * kTicketStride * sizeof(unsigned), s));
  HIPC(hipMemsetAsync(pt.red.ptr, 0, 16 * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.x.ptr, 0, 3 * N * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.p.ptr, 0, 3 * N * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.q.ptr, 0, 3 * N * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.stress.ptr, 0, E * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.val.ptr, 0, 6 * pt.G * sizeof(double), s));
  HIPC(hipMemsetAsync(pt.diag.ptr, 0, 6 * N * sizeof(double), s));
  if (h->active_host.size() == (size_t)h->Ecount) {
    if (dm) {
      act.resize(E);
      for (int64_t le = 0; le < E; ++le) act[le] = h->active_host[pt.plan.elem_g[le]];
    } else {
      act = h->active_host;
    }
    HIPC(h2d_async(h, pt.active.ptr, act.data(), E));
  } else {
    HIPC(hipMemsetAsync(pt.active.ptr, 1, E, s));
  }
  // wave-local lanes (single partition: falls back to the SELL kernel when a
  // row cannot be placed; partitioned: required)
  const std::string lerr = build_ell(P, pt.L, dm ? &pt.plan.elem_pair : nullptr);
  pt.ell_ok = lerr.empty() && (dm || P.n_free > 0);
  if (dm && !lerr.empty()) return fail(MFEA_EINVAL, "partition " + std::to_string(pt.rank) + ": " + lerr);
  if (pt.ell_ok) {
    const Ell& L = pt.L;
    const int64_t NL = L.n_lanes;
    code.resize(NL);
    for (int64_t l = 0; l < NL; ++l)
      code[l] = (L.code[l] & 0xFFFFFFu) | (uint32_t)(uint8_t)(int8_t)L.info[l] << 24;
    HIPC(pt.e_code.alloc(NL));
    HIPC(pt.e_partner.alloc(NL));
    HIPC(pt.e_lane_row.alloc(NL));
    HIPC(pt.e_src_pos.alloc(3 * NL));
    HIPC(pt.e_nbr_lane.alloc(3 * NL));
    HIPC(pt.e_f.alloc((kEllDoubles - 24) * NL + 24 * std::max<int64_t>(NL, L.n_hrec + 1)));
    HIPC(h2d_async(h, pt.e_code.ptr, code.data(), NL * sizeof(uint32_t)));
    // Halo record layout (ell.hip load_lane): compact (measured on one box:
    // C3 21.8 vs 23.7 µs per iteration, C2 41.6 vs 41.7 ms per step) or one
    // per lane (option "ell_compact" 0).  The device partner is the record the lane
    // fills: its mirror lane's record.
    pt.ell_hc = h->opt_ell_compact;
    push.resize(NL);
    for (int64_t l = 0; l < NL; ++l)
      push[l] = L.partner[l] >= 0 ? (pt.ell_hc ? L.hrec[L.partner[l]] : L.partner[l]) : L.partner[l];
    HIPC(h2d_async(h, pt.e_partner.ptr, push.data(), NL * sizeof(int32_t)));
    HIPC(pt.e_hmask.alloc(NL / 64));
    HIPC(pt.e_hbase.alloc(NL / 64));
    HIPC(h2d_async(h, pt.e_hmask.ptr, L.hmask.data(), NL / 64 * sizeof(uint64_t)));
    HIPC(h2d_async(h, pt.e_hbase.ptr, L.hbase.data(), NL / 64 * sizeof(int32_t)));
    HIPC(h2d_async(h, pt.e_lane_row.ptr, L.lane_row.data(), NL * sizeof(int32_t)));
    HIPC(h2d_async(h, pt.e_src_pos.ptr, L.src_pos.data(), 3 * NL * sizeof(int32_t)));
    HIPC(h2d_async(h, pt.e_nbr_lane.ptr, L.nbr_lane.data(), 3 * NL * sizeof(int32_t)));
    // zero records: a lane without a halo slot reads its neighbour's (unused)
    if (NL) HIPC(hipMemsetAsync(pt.e_f.ptr, 0, pt.e_f.n * sizeof(double), s));
  }
  if (dm) {
    const PartPlan& pl = pt.plan;
    const int64_t NX = std::max<int64_t>(pl.n_pairs, 1);
    HIPC(pt.xrec.alloc(4 * NX * kRecMax + NX * kMMax));
    pt.dv.xs[0] = pt.xrec.ptr;
    pt.dv.xs[1] = pt.xrec.ptr + NX * kRecMax;
    pt.dv.xr[0] = pt.xrec.ptr + 2 * NX * kRecMax;
    pt.dv.xr[1] = pt.xrec.ptr + 3 * NX * kRecMax;
    pt.dv.mr = pt.xrec.ptr + 4 * NX * kRecMax;
    HIPC(hipMemsetAsync(pt.xrec.ptr, 0, pt.xrec.n * sizeof(double), s));
    HIPC(pt.gbuf.alloc(2 * 4 * kMaxRanks + 4 + 4 * kMaxRanks));
    pt.dv.gall[0] = pt.gbuf.ptr;
    pt.dv.gall[1] = pt.gbuf.ptr + 4 * kMaxRanks;
    pt.dv.gsend = pt.gbuf.ptr + 8 * kMaxRanks;
    pt.gred = pt.gbuf.ptr + 8 * kMaxRanks + 4;
    HIPC(hipMemsetAsync(pt.gbuf.ptr, 0, pt.gbuf.n * sizeof(double), s));
    const int64_t ns = (int64_t)pl.xsend_node.size(), nr = (int64_t)pl.xrecv_node.size();
    HIPC(pt.xh.alloc(3 * (ns + nr)));
    pt.xh_send = pt.xh.ptr;
    pt.xh_recv = pt.xh.ptr + 3 * ns;
    rs.resize(ns);
    rr.resize(nr);
    for (int64_t i = 0; i < ns; ++i) rs[i] = P.iperm[pl.xsend_node[i]];
    for (int64_t i = 0; i < nr; ++i) rr[i] = P.iperm[pl.xrecv_node[i]];
    HIPC(pt.xsend_rows.alloc(ns));
    HIPC(pt.xrecv_rows.alloc(nr));
    HIPC(h2d_async(h, pt.xsend_rows.ptr, rs.data(), ns * sizeof(int32_t)));
    HIPC(h2d_async(h, pt.xrecv_rows.ptr, rr.data(), nr * sizeof(int32_t)));
    HIPC(pt.elem_own.alloc(E));
    HIPC(h2d_async(h, pt.elem_own.ptr, pl.elem_own.data(), E));
  }
  HIPC(pt.fail_list.alloc(std::max<int64_t>(E, 1)));
  HIPC(pt.fail_cnt.alloc(1));
  if (!dm) {
    HIPC(pt.event_of.alloc(std::max<int64_t>(E, 1)));
    HIPC(pt.eps.alloc(std::max<int64_t>(E, 1)));
    HIPC(hipMemsetAsync(pt.event_of.ptr, 0xFF, std::max<int64_t>(E, 1) * sizeof(int32_t), s));
  }
  HIPC(hipStreamSynchronize(s));
  return 0;
}

// Build the symbolic pattern(s) and (re)allocate + upload device state.
int ensure_built(mfea_handle* h) {
  if (!h->has_mesh) return fail(MFEA_ESTATE, "no mesh: call mfea_set_mesh first");
  if (!h->dirty) return 0;
  destroy_graph(h);
  h->assembled = false;
  h->gkey_gen = -1;
  const bool dm = h->world > 1 || h->nparts > 1;
  if (dm && h->has_props())
    return fail(MFEA_ESTATE, "per-element properties: one partition per handle (mfea_set_element_props(h, NULL) first)");
  if (dm && h->bc.field.set)
    return fail(MFEA_ESTATE, "grip field: one partition per handle (mfea_set_grip_field(h, NULL) first)");
  if (dm && h->bc.loads.set)
    return fail(MFEA_ESTATE, "nodal loads: one partition per handle (mfea_set_node_loads(h, NULL, 0) first)");
  if (dm && !h->bc.grip_default())
    return fail(MFEA_ESTATE, "grip motion: one partition per handle (set the directions (0,1,0), (0,1,0) first)");
  const int np = h->world > 1 ? 1 : h->nparts;
  const bool skip = (h->mesh_flags & MFEA_MESH_SKIP_INVALID) != 0;
  h->parts.clear();
  for (int i = 0; i < np; ++i) {
    h->parts.push_back(std::make_unique<Part>());
    Part& pt = *h->parts.back();
    pt.rank = h->world > 1 ? h->rank : i;
    std::string err;
    if (!dm) {
      err = build_pattern(h->N, h->xyz.data(), h->Ecount, h->e2n.data(), skip, h->top, h->bot,
                          order_mode(h), pt.P);
    } else {
      err = build_partition(h->N, h->xyz.data(), h->Ecount, h->e2n.data(), skip, h->top, h->bot,
                            h->world > 1 ? h->world : np, pt.rank, h->axis, h->opt_part_slack, pt.plan);
      if (err.empty())
        err = build_pattern((int64_t)pt.plan.node_g.size(), pt.plan.xyz.data(),
                            (int64_t)pt.plan.elem_g.size(), pt.plan.e2n.data(), false, pt.plan.top,
                            pt.plan.bot, order_mode(h), pt.P, &pt.plan.ghost);
    }
    if (!err.empty()) {
      h->parts.resize(1);
      return fail(MFEA_EINVAL, err);
    }
    if (i == 0) {
      pt.mirror = h->d_host_state;
    } else {
      HIPC(pt.state_mirror.alloc(1));
      pt.mirror = pt.state_mirror.ptr;
    }
    RC(upload_part(h, pt, dm));
    if (h->bc.field.set) RC(upload_field(h, pt));
    if (h->bc.loads.set) RC(upload_loads(h, pt));
  }
  if (dm) {  // distributed GAMG: the whole mesh's pattern and the node owners
    h->gamg_ok = false;
    h->gamg = AmgPlan();
    h->gowner = part0(h).plan.owner;
    const std::string err = build_pattern(h->N, h->xyz.data(), h->Ecount, h->e2n.data(), skip, h->top, h->bot,
                                          order_mode(h), h->gpat);
    if (!err.empty()) return fail(MFEA_EINVAL, err);
  } else {
    h->gpat = Pattern();
  }
  ++h->act_gen;
  ++h->act_sub_gen;
  {  // free DOFs of the whole mesh (reported in mfea_stats)
    std::vector<uint8_t> known(h->N, 0);
    for (int64_t t : h->top) known[t] = 1;
    for (int64_t b : h->bot) known[b] = 1;
    h->n_free_global = h->N - (int64_t)std::count(known.begin(), known.end(), 1);
  }
  if (!dm) {  // the host view of the activity the device now holds
    const int64_t E = part0(h).P.n_elems;
    if (h->active_host.size() == (size_t)h->Ecount) {
      h->act_host.resize(E);
      for (int64_t e = 0; e < E; ++e) h->act_host[e] = h->active_host[e] ? 1 : 0;
    } else {
      h->act_host.assign(E, 1);
    }
    h->act_count = (int64_t)std::count(h->act_host.begin(), h->act_host.end(), (uint8_t)1);
    h->act_host_ok = true;
    // (the count the first post will report: it only moves act_gen, and with
    // it the kept K, when elements did fail)
    h->n_active = h->act_count;
  }
  h->active_host.clear();
  h->dirty = false;
  return 0;
}

// The lane operator pays off while most rows fit one lane.  Dense networks
// (C5: mean degree 7.5 → 4.5 lanes per free row, most of them helpers that
// move zeros) run the SELL kernel instead: measured 0.94 vs 2.16 ms per
// iteration at 10 M DOF.  The partitioned path always runs lanes.
// Option "cg_kernel" 1 (lanes) / 2 (SELL) forces one (comparison runs).
bool use_ell(const mfea_handle* h, const Part& pt) {
  if (!pt.ell_ok) return false;
  if (h->opt_cg_kernel == 2) return false;
  if (h->opt_cg_kernel == 1) return true;
  return pt.L.n_lanes <= 2 * std::max<int64_t>(pt.P.n_free, 1);
}

mfea_solve_opts default_opts() {
  mfea_solve_opts o;
  o.rtol = 1e-5;
  o.atol = 1e-50;
  o.max_it = 10000;
  o.precond = MFEA_PC_JACOBI;
  o.norm = MFEA_NORM_UNPRECONDITIONED;
  o.chunk = 0;
  o.reg = 1e-12;
  return o;
}

SellOp sell_op(Part& pt) {
  SellOp op;
  op.N = pt.P.n_nodes;
  op.nf = pt.P.n_free;
  op.G = pt.G;
  op.slice_ptr = pt.slice_ptr.ptr;
  op.row_len = pt.row_len.ptr;
  op.s_col = pt.s_col.ptr;
  op.val = pt.val.ptr;
  op.diag = pt.diag.ptr;
  return op;
}

CgVecs cg_vecs(Part& pt) {
  CgVecs v;
  v.x = pt.x.ptr;
  v.p = pt.p.ptr;
  v.r[0] = pt.r.ptr;
  v.r[1] = pt.cg_r1.ptr;
  v.s[0] = pt.cg_s0.ptr;
  v.s[1] = pt.cg_s1.ptr;
  v.w[0] = pt.cg_w0.ptr;
  v.w[1] = pt.cg_w1.ptr;
  v.dinv = pt.dinv.ptr;
  return v;
}

// stride of the halo record arrays: compact records + a spare, or one per lane
int64_t ell_nr(const Part& pt) { return pt.ell_hc ? pt.L.n_hrec + 1 : pt.L.n_lanes; }

EllOp ell_op(const mfea_handle* h, Part& pt) {
  EllOp op;
  const int64_t NL = pt.L.n_lanes;
  op.NL = NL;
  op.nd = lane_dofs(h);
  op.code = pt.e_code.ptr;
  op.partner = pt.e_partner.ptr;
  op.lane_row = pt.e_lane_row.ptr;
  op.src_pos = pt.e_src_pos.ptr;
  op.nbr_lane = pt.e_nbr_lane.ptr;
  op.V = pt.e_f.ptr;
  op.D = op.V + 18 * NL;
  op.hc = pt.ell_hc ? 1 : 0;
  op.NR = ell_nr(pt);
  op.hmask = pt.e_hmask.ptr;
  op.hbase = pt.e_hbase.ptr;
  op.bs = h->opt_ell_block;
  op.maxg = h->opt_ell_maxg;
  return op;
}

EllVecs ell_vecs(Part& pt) {
  EllVecs v;
  const int64_t NL = pt.L.n_lanes;
  double* f = pt.e_f.ptr + 24 * NL;
  auto take = [&](int64_t n) {
    double* p = f;
    f += n * NL;
    return p;
  };
  v.x = take(3);
  v.p = take(3);
  for (int q = 0; q < 2; ++q) {
    v.r[q] = take(3);
    v.s[q] = take(3);
    v.w[q] = take(3);
  }
  v.M = take(6);
  const int64_t NR = ell_nr(pt);
  v.h[0] = f;
  v.h[1] = f + 9 * NR;
  v.hM = f + 18 * NR;
  return v;
}

// ---------------------------------------------------------------------------
// Exchanges of the partitioned solve.  Over RCCL: ONE group of point-to-point
// transfers per exchange point on the handle's stream — the neighbour
// payloads and the 4 partial sums to every other rank (send/recv pairs, not a
// ring all-gather: over xGMI every rank pair has its own link, so the sums
// cost one hop instead of world − 1 ring steps).  The sums travel as copies:
// every rank then adds the same bits in the same (rank) order — never an
// all-reduce, whose summation order may differ per rank.  The producer of
// gsend also writes the rank's own row of gall[q].
// Partitions on one device: device copies on the same stream.
// ---------------------------------------------------------------------------
// inside an open group: gsend → row `rank` of every other rank's gall
int sums_p2p(mfea_handle* h, const double* gsend, double* gall) {
  for (int r = 0; r < h->world; ++r) {
    if (r == h->rank) continue;
    NCCLC(ncclSend(gsend, 4, ncclFloat64, r, h->comm, h->stream));
    NCCLC(ncclRecv(gall + 4 * r, 4, ncclFloat64, r, h->comm, h->stream));
  }
  return 0;
}

// CG records of parity q (xs[q] → the peers' xr[q]); gather: this rank's
// partial sums (gsend) → row `rank` of every rank's gall[q]
int xchg_records(mfea_handle* h, int q, bool gather) {
  const int64_t RW = 3 * lane_dofs(h);
  hipStream_t s = h->stream;
  if (h->world > 1) {
    Part& pt = part0(h);
    const PartPlan& pl = pt.plan;
    if (pl.peers.empty() && !gather) return 0;
    NCCLC(ncclGroupStart());
    for (size_t i = 0; i < pl.peers.size(); ++i) {
      const size_t n = (size_t)(pl.peer_cnt[i] * RW);
      NCCLC(ncclSend(pt.dv.xs[q] + pl.peer_off[i] * RW, n, ncclFloat64, pl.peers[i], h->comm, s));
      NCCLC(ncclRecv(pt.dv.xr[q] + pl.peer_off[i] * RW, n, ncclFloat64, pl.peers[i], h->comm, s));
    }
    if (gather) RC(sums_p2p(h, pt.dv.gsend, pt.dv.gall[q]));
    NCCLC(ncclGroupEnd());
    return 0;
  }
  for (auto& a : h->parts) {
    const PartPlan& pa = a->plan;
    for (size_t i = 0; i < pa.peers.size(); ++i) {
      Part& b = *h->parts[pa.peers[i]];
      const PartPlan& pb = b.plan;
      const auto it = std::lower_bound(pb.peers.begin(), pb.peers.end(), a->rank);
      const size_t jb = (size_t)(it - pb.peers.begin());
      if (it == pb.peers.end() || *it != a->rank || pb.peer_cnt[jb] != pa.peer_cnt[i])
        return fail(MFEA_EINVAL, "internal: asymmetric exchange plan");
      HIPC(hipMemcpyAsync(b.dv.xr[q] + pb.peer_off[jb] * RW, a->dv.xs[q] + pa.peer_off[i] * RW,
                          pa.peer_cnt[i] * RW * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (gather)
      for (auto& b : h->parts)
        if (b != a)
          HIPC(hipMemcpyAsync(b->dv.gall[q] + 4 * a->rank, a->dv.gsend, 4 * sizeof(double),
                              hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// displacement halo: xh_send (packed owned rows) → the peers' xh_recv
int xchg_xhalo(mfea_handle* h) {
  hipStream_t s = h->stream;
  if (h->world > 1) {
    Part& pt = part0(h);
    const PartPlan& pl = pt.plan;
    NCCLC(ncclGroupStart());
    for (size_t i = 0; i < pl.xpeers.size(); ++i) {
      if (pl.xsend_cnt[i])
        NCCLC(ncclSend(pt.xh_send + 3 * pl.xsend_off[i], (size_t)(3 * pl.xsend_cnt[i]), ncclFloat64,
                       pl.xpeers[i], h->comm, s));
      if (pl.xrecv_cnt[i])
        NCCLC(ncclRecv(pt.xh_recv + 3 * pl.xrecv_off[i], (size_t)(3 * pl.xrecv_cnt[i]), ncclFloat64,
                       pl.xpeers[i], h->comm, s));
    }
    NCCLC(ncclGroupEnd());
    return 0;
  }
  for (auto& a : h->parts) {
    const PartPlan& pa = a->plan;
    for (size_t i = 0; i < pa.xpeers.size(); ++i) {
      if (!pa.xsend_cnt[i]) continue;
      Part& b = *h->parts[pa.xpeers[i]];
      const PartPlan& pb = b.plan;
      const auto it = std::lower_bound(pb.xpeers.begin(), pb.xpeers.end(), a->rank);
      const size_t jb = (size_t)(it - pb.xpeers.begin());
      if (it == pb.xpeers.end() || *it != a->rank || pb.xrecv_cnt[jb] != pa.xsend_cnt[i])
        return fail(MFEA_EINVAL, "internal: asymmetric displacement halo");
      HIPC(hipMemcpyAsync(b.xh_recv + 3 * pb.xrecv_off[jb], a->xh_send + 3 * pa.xsend_off[i],
                          3 * pa.xsend_cnt[i] * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
  }
  return 0;
}

// 4 doubles at red + off of every partition → row `rank` of every gred
int gather4(mfea_handle* h, int off) {
  hipStream_t s = h->stream;
  if (h->world > 1) {
    Part& pt = part0(h);
    NCCLC(ncclAllGather(pt.red.ptr + off, pt.gred, 4, ncclFloat64, h->comm, s));
    return 0;
  }
  for (auto& a : h->parts)
    for (auto& b : h->parts)
      HIPC(hipMemcpyAsync(b->gred + 4 * a->rank, a->red.ptr + off, 4 * sizeof(double),
                          hipMemcpyDeviceToDevice, s));
  return 0;
}

// ---------------------------------------------------------------------------
// enqueue one chunk of single-reduction CG iterations (one kernel each)
void enqueue_chunk(mfea_handle* h, int chunk, int precond, bool ell) {
  hipStream_t s = h->stream;
  Part& pt = part0(h);
  if (ell) {
    const EllOp op = ell_op(h, pt);
    const EllVecs v = ell_vecs(pt);
    for (int j = 0; j < chunk; ++j)
      launch_ell_iter(s, j, op, precond, v, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr);
  } else {
    const SellOp op = sell_op(pt);
    const CgVecs v = cg_vecs(pt);
    for (int j = 0; j < chunk; ++j)
      launch_cg_iter(s, j, op, precond, v, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr);
  }
  launch_cg_advance(s, chunk, pt.slots.ptr, pt.state.ptr, pt.mirror);
}

// partitioned: per iteration, every partition's iteration kernel, its partial
// sums, then one exchange of records + sums (launched eagerly)
int enqueue_chunk_dist(mfea_handle* h, int chunk, int precond) {
  hipStream_t s = h->stream;
  for (int j = 0; j < chunk; ++j) {
    const int q = (j & 1) ^ 1;
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_ell_iter(s, j, ell_op(h, pt), precond, ell_vecs(pt), pt.slots.ptr, pt.state.ptr,
                      pt.cg_part.ptr, nullptr, &pt.dv);
    }
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_psum(s, ell_op(h, pt), cg_part_buf(pt, q), pt.dv.gall[q] + 4 * pt.rank, pt.dv.gsend);
    }
    HIPC(hipGetLastError());
    RC(xchg_records(h, q, true));
  }
  for (auto& pp : h->parts) launch_cg_advance(s, chunk, pp->slots.ptr, pp->state.ptr, pp->mirror);
  HIPC(hipGetLastError());
  return 0;
}

// Replays chunks until the device reports done; at most two chunks in flight.
// mirror = true: the chunk's advance kernel writes the final state into the
// mapped pinned h_state[0] itself (CG-CG path); otherwise copy it per chunk.
template <class Enqueue>
int drive_chunks(mfea_handle* h, int chunk, int max_it, Enqueue&& enqueue, SolveState* out,
                 bool mirror = false) {
  hipStream_t s = h->stream;
  Part& pt = part0(h);
  const int64_t max_chunks = (int64_t)max_it / chunk + 3;
  int64_t k = 0;
  bool done = false;
  volatile SolveState* hs = h->h_state;
  if (mirror) hs[0].done = 0;
  while (!done && k < max_chunks) {
    int rc = enqueue();
    if (rc) return rc;
    if (!mirror)
      HIPC(hipMemcpyAsync(&h->h_state[k & 1], pt.state.ptr, sizeof(SolveState),
                          hipMemcpyDeviceToHost, s));
    HIPC(hipEventRecord(h->poll[k & 1], s));
    if (k >= 1) {
      RC(wait_event(h, h->poll[(k - 1) & 1]));
      if (hs[mirror ? 0 : (k - 1) & 1].done) done = true;
    }
    ++k;
  }
  RC(sync_stream(h));
  const SolveState& last = h->h_state[mirror ? 0 : (k - 1) & 1];
  if (!last.done) {
    // should not happen (max_chunks covers max_it); report as maxit
    *out = last;
    out->status = MFEA_EMAXIT;
    out->iters = max_it;
    return 0;
  }
  *out = last;
  return 0;
}

// Replays planned from the expected iteration count (the AMG solves of one
// handle converge in a near-constant number of iterations): enough chunks
// for `expected` iterations are queued back to back with no host wait, then
// one chunk at a time until the device reports done.  A wrong guess costs a
// chunk of early-exiting launches (too high) or one host round trip per
// extra chunk (too low) — never correctness.  `after` is queued behind every
// batch before the host waits (the solve's epilogue: if that batch
// converged, the stream is already past it when the host wakes; if not, the
// next batch's copy supersedes it).
struct NoEpilogue {
  int operator()() const { return 0; }
};
template <class Enqueue, class After = NoEpilogue>
int drive_planned(mfea_handle* h, int chunk, int max_it, int expected, Enqueue&& enqueue,
                  SolveState* out, After&& after = After{}) {
  hipStream_t s = h->stream;
  const int64_t max_chunks = (int64_t)max_it / chunk + 3;
  volatile SolveState* hs = h->h_state;
  hs[0].done = 0;
  int64_t k = 0;
  const int64_t first = std::min<int64_t>(max_chunks, std::max(1, (expected + 1 + chunk - 1) / chunk));
  for (; k < first; ++k) RC(enqueue());
  RC(after());
  HIPC(hipEventRecord(h->poll[0], s));
  RC(wait_event(h, h->poll[0]));
  while (!hs[0].done && k < max_chunks) {
    RC(enqueue());
    RC(after());
    HIPC(hipEventRecord(h->poll[0], s));
    RC(wait_event(h, h->poll[0]));
    ++k;
  }
  RC(sync_stream(h));
  *out = h->h_state[0];
  if (!out->done) {
    out->status = MFEA_EMAXIT;
    out->iters = max_it;
  }
  return 0;
}

// drive_planned with chunks of two sizes: the planned batch (`expected`
// updates) as long chunks of `big` iterations plus short ones of `small` for
// the remainder — one chunk boundary (advance kernel + graph-to-graph gap,
// ≈ 13 µs) per `big` iterations instead of per `small`, while a batch never
// overshoots the expected count by more than small − 1 — then short chunks
// one at a time until the device reports done.  enqueue(size) queues one.
// zero_ok (chunks that end with a closing check, enqueue_amg_chunk): a batch
// of no updates is queued as one chunk of length 0 — the check alone.
template <class Enqueue, class After = NoEpilogue>
int drive_sized(mfea_handle* h, int big, int small, int max_it, int expected, Enqueue&& enqueue,
                SolveState* out, After&& after = After{}, bool exact_rem = false, bool zero_ok = false) {
  hipStream_t s = h->stream;
  volatile SolveState* hs = h->h_state;
  hs[0].done = 0;
  const int need = std::max(zero_ok ? 0 : 1, expected + 1);  // updates the batch assumes, as drive_planned
  if (need == 0) RC(enqueue(0));
  const int nbig = big > small ? need / big : 0;
  const int rem = need - nbig * big;
  const int nsmall = (rem + small - 1) / small;
  int64_t done_its = 0;
  for (int k = 0; k < nbig; ++k, done_its += big) RC(enqueue(big));
  if (exact_rem && rem > 0) {  // one chunk of the remainder's own length (drive_rem_chunk)
    RC(enqueue(rem));
    done_its += rem;
  } else {
    for (int k = 0; k < nsmall; ++k, done_its += small) RC(enqueue(small));
  }
  RC(after());
  HIPC(hipEventRecord(h->poll[0], s));
  RC(wait_event(h, h->poll[0]));
  while (!hs[0].done && done_its < (int64_t)max_it + 3 * small) {
    RC(enqueue(small));
    RC(after());
    HIPC(hipEventRecord(h->poll[0], s));
    RC(wait_event(h, h->poll[0]));
    done_its += small;
  }
  RC(sync_stream(h));
  *out = h->h_state[0];
  if (!out->done) {
    out->status = MFEA_EMAXIT;
    out->iters = max_it;
  }
  return 0;
}

// mfea_step's planned batch as one graph (solve_amg, option batch_graph):
// the batch's iterations, the finish and the post; the post counts as the
// step's speculative post (mfea_handle::spec_used), so when the solve goes on
// in small chunks their first batch end undoes its failures (spec_post)
template <class Launch, class Enqueue, class After>
int drive_batch(mfea_handle* h, int small, int max_it, int need, Launch&& launch, Enqueue&& enqueue,
                SolveState* out, After&& after, bool launched = false) {
  hipStream_t s = h->stream;
  volatile SolveState* hs = h->h_state;
  if (!launched) hs[0].done = 0;
  RC(launch());
  h->spec_used = true;
  h->spec_launched = true;
  HIPC(hipEventRecord(h->ev[5], s));  // the post's read-back: the end of the batch
  HIPC(hipEventRecord(h->poll[0], s));
  RC(wait_event(h, h->poll[0]));
  int64_t done_its = need;
  while (!hs[0].done && done_its < (int64_t)max_it + 3 * small) {
    RC(enqueue(small));
    RC(after());
    HIPC(hipEventRecord(h->poll[0], s));
    RC(wait_event(h, h->poll[0]));
    done_its += small;
  }
  RC(sync_stream(h));
  *out = h->h_state[0];
  if (!out->done) {
    out->status = MFEA_EMAXIT;
    out->iters = max_it;
  }
  return 0;
}

// device times of the last solve (its events must have completed)
void solve_times(mfea_handle* h, mfea_stats* st) {
  if (!h->opt_phase_times) return;  // (no phase events recorded: the t_* stay 0)
  float ms = 0;
  (void)hipEventElapsedTime(&ms, h->ev[1], h->ev[2]);
  st->t_rhs_ms = ms;
  (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]);
  st->t_solve_ms = ms;
  if (h->ev_setup_used) {
    (void)hipEventElapsedTime(&ms, h->ev[2], h->ev_setup);
    st->t_setup_ms = h->setup_skipped ? 0.0 : ms;  // (kept values: the event is recorded, nothing ran before it)
  }
}

// The solve's end: the status comes from the host copy of the final state
// (drive_chunks / drive_planned waited for it); inside mfea_step the stream
// is not waited for here — post's wait covers it and the times are read then
// (one host round trip less per step).
int finish_solve(mfea_handle* h, const SolveState& fin, mfea_stats* st) {
  if (!h->in_step) {  // (mfea_solve: its end is waited for here)
    HIPC(hipEventRecord(h->ev[3], h->stream));
    RC(wait_event(h, h->ev[3]));
  } else if (!h->spec_launched) {  // (a speculative post recorded it before itself)
    RC(phase_event(h, h->ev[3], h->stream));
  }
  if (st) {
    st->iters = fin.iters;
    st->status = fin.status;
    st->bnorm = std::sqrt(fin.bb0);
    st->relres = fin.res0 > 0 ? std::sqrt(fin.res_final / fin.res0) : 0.0;
    st->n_free = 3 * h->n_free_global;
    if (!h->in_step) solve_times(h, st);
  }
  if (fin.status == -4) return fail(MFEA_EMAXIT, "PCG reached max_it without converging");
  if (fin.status == -5) return fail(MFEA_EBREAKDOWN, "PCG breakdown (p·Ap <= 0 or non-finite)");
  return 0;
}

int solve_chunk_size(const mfea_solve_opts* o) {
  int chunk = o->chunk > 0 ? std::min(o->chunk, kMaxChunk) : 32;
  return chunk + (chunk & 1);  // even: the iteration kernels take the buffer parity from j
}

int solve_impl(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o,
               mfea_stats* st) {
  Part& pt = part0(h);
  hipStream_t s = h->stream;
  const int precond = o->precond == MFEA_PC_BLOCK_JACOBI ? 1 : 0;
  const int chunk = solve_chunk_size(o);
  const SellOp op = sell_op(pt);
  const CgVecs v = cg_vecs(pt);
  RC(phase_event(h, h->ev[1], s));
  launch_cg_rhs(s, op, pt.code.ptr, dy_top, dy_bot, o->reg, precond, v, pt.partials.ptr, tix(pt, 0),
                pt.red.ptr, h->bc.form(pt));
  launch_cg_init_finalize(s, pt.red.ptr, o->rtol, o->atol, o->norm, o->max_it, o->reg,
                          pt.state.ptr,
                          pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
  const bool ell = use_ell(h, pt);
  if (ell) {
    launch_ell_init(s, ell_op(h, pt), op, precond, v, ell_vecs(pt));
    launch_ell_first(s, ell_op(h, pt), o->reg, precond, ell_vecs(pt), pt.slots.ptr, pt.cg_part.ptr);
  } else {
    launch_cg_first(s, op, o->reg, precond, v, pt.slots.ptr, pt.cg_part.ptr);
  }
  HIPC(hipGetLastError());
  RC(phase_event(h, h->ev[2], s));
  // option "graph" 0: launch the chunk kernels eagerly (profilers that do not
  // follow hipGraph replays; same kernels, same order)
  const bool no_graph = !h->opt_graph;
  SolveState fin;
  int rc;
  if (no_graph) {
    rc = drive_chunks(
        h, chunk, o->max_it,
        [&]() -> int {
          enqueue_chunk(h, chunk, precond, ell);
          HIPC(hipGetLastError());
          return 0;
        },
        &fin, /*mirror=*/true);
  } else {
    if (h->graph == nullptr || h->graph_chunk != chunk || h->graph_precond != precond ||
        h->graph_ell != (ell ? lane_dofs(h) : 0)) {
      destroy_graph(h);
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      enqueue_chunk(h, chunk, precond, ell);
      HIPC(hipStreamEndCapture(s, &g));
      hipError_t e = hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      h->graph_chunk = chunk;
      h->graph_precond = precond;
      h->graph_ell = ell ? lane_dofs(h) : 0;
    }
    rc = drive_chunks(
        h, chunk, o->max_it,
        [&]() -> int {
          HIPC(hipGraphLaunch(h->graph, s));
          return 0;
        },
        &fin, /*mirror=*/true);
  }
  if (rc) return rc;
  if (ell) {
    launch_ell_finish(s, ell_op(h, pt), ell_vecs(pt), pt.x.ptr);
    HIPC(hipGetLastError());
  }
  return finish_solve(h, fin, st);
}

// ---------------------------------------------------------------------------
// SA-AMG preconditioned CG (amg.hpp / amg.hip), single partition.
// ---------------------------------------------------------------------------
// rows [lo, hi) of a SELL pattern and their positions (amg_kernels.hpp RowRange)
RowRange row_range(const SellPat& S, int64_t lo, int64_t hi) {
  RowRange g;
  g.lo = lo;
  g.hi = hi > lo ? hi : lo;
  if (hi <= lo || S.sptr.size() < 2) return g;
  g.s0 = lo >> 6;
  g.s1 = (hi - 1) >> 6;
  g.p0 = (int64_t)S.sptr[g.s0] * 64;
  g.p1 = (int64_t)S.sptr[g.s1 + 1] * 64;
  g.pf = (int64_t)S.sptr[g.s0 + 1] * 64;
  g.pl = (int64_t)S.sptr[g.s1] * 64;
  return g;
}

// Carves the plan's index arrays and the value / vector arrays out of two
// device allocations and uploads the indices (carve.hpp, stage_flush).  Pass 0
// sizes, pass 1 carves.
// rk (distributed GAMG): this partition's row ranges, with its own level-0
// lists over ITS pattern (a0, row0) in place of the plan's.
// strength of connection of the level-0 aggregation (option amg_theta_ppm;
// amg.hpp AmgStrength): θ and the bending-to-axial constant 12EI / EA
AmgStrength amg_strength(const mfea_handle* h) {
  AmgStrength st;
  st.theta = h->opt_amg_theta_ppm * 1e-6;
  st.kb_kax = h->mat.EA > 0.0 ? h->mat.EI12 / h->mat.EA : 0.0;
  st.sec = h->pe_sec.empty() ? nullptr : h->pe_sec.data();  // (one partition: element ids are the pattern's)
  return st;
}

// w = A u's step width: K = 2 (slices up to 2U blocks in one round trip of
// column loads and gathers, more VGPRs) once level 0's mean slice width
// passes U = 4 blocks, or on a small network, whose launch is one chain of
// dependent loads long and ends with its widest slices (C2 iteration 26.1 →
// 25.4 µs; C3 66.6 vs 66.8, kept at K = 1: profiles/r5/ab_spmv_k.jsonl)
constexpr int64_t kWideSpmvRows = 131072;
static int amg_w_k(const AmgPlan& pl) {
  if (pl.lev.empty() || pl.lev[0].A.sptr.size() < 2) return 1;
  const auto& sp = pl.lev[0].A.sptr;
  const double mean = (double)(sp.back() - sp.front()) / (double)(sp.size() - 1);
  return mean > 4.0 || pl.lev[0].A.n <= kWideSpmvRows ? 2 : 1;
}

// the collapsed cycle's lowest level when chosen automatically: level 1's V
// is dense-ish on small networks (the reference network: 80 blocks per row,
// 0.3 M product pairs, a few ms of host build per rebuild) for one saved
// launch pair; level 2 is what C2 / C3 choose anyway
constexpr int kAmgCollapseAutoLevel = 2;
constexpr int64_t kMergeRows = 131072;  // amg_merge -1: level-0 rows up to which levels 0 and 1 merge

// Level 0's up sweep and w = A u in one launch (option amg_fuse_l0; DESIGN.md
// §4.12): what −1 means, and the level-0 window the fused plans are built at
constexpr bool kAmgFuseAuto = true;
constexpr int64_t kAmgFuseWindow = 1408;
bool amg_fuse_opted(const mfea_handle* h) { return h->opt_amg_fuse_l0 > 0 || (h->opt_amg_fuse_l0 < 0 && kAmgFuseAuto); }
// … wanted for a plan still to be built: one partition, GAMG's compact cycle,
// and not a network whose levels 0 and 1 merge (those keep their launches)
bool amg_fuse_wanted(const mfea_handle* h, const Part& pt, int kind) {
  if (!amg_fuse_opted(h) || partitioned(h) || kind != MFEA_PC_GAMG || h->opt_amg_cycle != 1) return false;
  return !(h->opt_amg_merge > 0 || (h->opt_amg_merge < 0 && pt.P.n_free <= kMergeRows));
}
int64_t amg_l0_window(const mfea_handle* h, const Part& pt, int kind) {
  if (h->opt_amg_l0_window > 0) return h->opt_amg_l0_window;
  return amg_fuse_wanted(h, pt, kind) ? kAmgFuseWindow : kAmgSortWindow;
}

// ρ̂ of the levels below 0 (0: the Gershgorin rule), until a solve has failed
// with it
double coarse_rho(const mfea_handle* h) {
  return h->amg_safe_omega ? 0.0 : (double)h->opt_amg_coarse_rho_ppm * 1e-6;
}

// The smoothing weights of a partition's hierarchy for the handle's current
// mode (DESIGN.md §4.2 "Coarse-level smoothing weight"): over-relaxed — ρ̂_l
// fixed at coarse_rho below level 0 and at 2 (its exact bound) on level 0,
// so no Gershgorin pass and, on an own hierarchy, no coarse D⁻¹ launches
// (fixed_omega) — or, after a fallback, the Gershgorin-safe rule (omega[0] =
// 0: the setup estimates ρ̂_l).  Called at upload and whenever the mode
// changes; the next numeric setup re-forms every ω product.
int apply_coarse_omega(mfea_handle* h, Part& pt) {
  hipStream_t s = h->stream;
  const int nlev = (int)pt.amg_lev.size();
  const double rho = coarse_rho(h);
  static const double kRho0 = 2.0;
  pt.kept.ok = false;  // (the kept values hold the old weights' products)
  for (int l = 0; l < nlev; ++l) {
    AmgLevD& d = pt.amg_lev[l];
    d.fixed_omega = pt.amg_om_own && l > 0 && rho > 0.0 ? 1 : 0;
    d.a0full = 0;
    d.a0slot = l == 0 ? h->opt_amg_a0_slot : 0;
    HIPC(hipMemsetAsync(d.omega, 0, sizeof(double), s));
    if (l > 0 && rho > 0.0) HIPC(hipMemcpyAsync(d.omega, &rho, sizeof(double), hipMemcpyHostToDevice, s));
  }
  // level 0: its P_0 / Ã_0 then come with A_0 in one row pass (k_amg_a0full)
  // where that measured faster: the Z-ordered plans (C5 setup 4.17 → 3.88
  // ms); on depth-first ones the per-position launch stays (C3 0.401 vs
  // 0.408 ms, C2 0.219 vs 0.224)
  if (pt.amg_om_own && nlev > 1 && rho > 0.0 && pt.amg_lev[0].compact) {
    pt.amg_lev[0].fixed_omega = 1;
    pt.amg_lev[0].a0full = pt.amg_om_spatial ? 1 : 0;
    HIPC(hipMemcpyAsync(pt.amg_lev[0].omega, &kRho0, sizeof(double), hipMemcpyHostToDevice, s));
  }
  if (nlev) {
    HIPC(pt.amg_levd.alloc(nlev));
    HIPC(hipMemcpyAsync(pt.amg_levd.ptr, pt.amg_lev.data(), nlev * sizeof(AmgLevD), hipMemcpyHostToDevice, s));
  }
  HIPC(hipStreamSynchronize(s));
  return 0;
}

// A GAMG solve that failed with the over-relaxed coarse smoothers may have
// met an operator on which they do not give an SPD cycle (ω_l λ_l ≥ 2).  A
// breakdown suggests that; max_it only when the caller's limit is far above
// what this hierarchy needs (`typical` iterations) — a deliberately small
// max_it is not ω's fault.
bool omega_suspect(const mfea_handle* h, int status, int max_it, int typical) {
  if (status == 0 || coarse_rho(h) <= 0.0) return false;
  if (status == -5) return true;
  return status == -4 && max_it > 4 * std::max(typical, 16);
}

// ... then the solve runs once more on the Gershgorin-safe weights, which stay
// for the handle's lifetime only if that solve converges; otherwise the
// over-relaxed ones come back and the retry's failure is returned.
// Partitioned over RCCL every rank sees the same status (the CG scalars are
// all-reduced), so every rank takes this path together.
template <class F>
int omega_retry(mfea_handle* h, F&& again) {
  RC(sync_stream(h));
  h->amg_safe_omega = true;
  for (auto& pp : h->parts) RC(apply_coarse_omega(h, *pp));
  const int rc = again();
  if (rc == MFEA_EMAXIT || rc == MFEA_EBREAKDOWN) {
    h->amg_safe_omega = false;
    for (auto& pp : h->parts) RC(apply_coarse_omega(h, *pp));
  }
  return rc;
}

// the merged cycle on or off (built plans only): level 2's x / e point into
// the merged vector buffer while on
void set_merge(mfea_handle* h, Part& pt) {
  const bool on = pt.amg_mplan.on && h->opt_amg_merge != 0 && pt.amg_lev.size() >= 4 && pt.amg_cg.coll == 2;
  pt.amg_mg.on = on ? 1 : 0;
  if (pt.amg_lev.size() > 2) {
    AmgLevD& L2 = pt.amg_lev[2];
    const int nd = pt.amg.nd;
    L2.x = on ? pt.amg_mg.B + (size_t)nd * pt.amg_mg.n1 : pt.amg_x2;
    L2.e = on ? pt.amg_mg.B + (size_t)nd * (pt.amg_mg.n1 + pt.amg_mg.n2) : pt.amg_e2;
  }
}

int upload_amg(mfea_handle* h, Part& pt, const AmgPlan& pl, const AmgRank* rk = nullptr,
               const PosList* a0 = nullptr, const std::vector<int32_t>* row0 = nullptr) {
  const int nd = pl.nd, nb2 = nd * nd;
  const int nlev = (int)pl.lev.size();
  hipStream_t s = h->stream;
  size_t ndd = 0, nff = 0;
  pt.amg_coll = AmgCollapse();
  // (a distributed plan: collapsed among its replicated levels only)
  if ((!rk || rk->compact) && h->opt_amg_cycle == 1 && h->opt_amg_collapse != 0) {
    const int min_level = h->opt_amg_collapse < 0 ? kAmgCollapseAutoLevel : std::max(1, h->opt_amg_collapse);
    const std::string cerr = build_amg_collapse(pl, h->opt_amg_collapse_mb << 20, h->opt_amg_collapse_pairs,
                                                rk ? std::max(min_level, rk->n_dist) : min_level, pt.amg_coll);
    if (!cerr.empty()) return fail(MFEA_EINVAL, cerr);
  }
  // levels 0 and 1 merged (amg.hpp AmgMerge): where the launches are latency-
  // bound — level 0 under kMergeRows rows (C2: 34 k; C3's 336 k measured
  // slower merged: its c_1 / x_2 / W rows add more bytes than two launches cost)
  pt.amg_mplan = AmgMerge();
  if (!rk && h->opt_amg_merge != 0 && pt.amg_coll.kc == 2 && nlev >= 4 &&
      (h->opt_amg_merge > 0 || pl.lev[0].A.n <= kMergeRows)) {
    const std::string merr = build_amg_merge(pl, pt.amg_coll, pt.amg_mplan);
    if (!merr.empty()) return fail(MFEA_EINVAL, merr);
  }
  // level 0 in tiles of its sorting window (AmgCg::w_tile) and the block halo
  // plan over them: one partition's GAMG hierarchy whose window is a tile size
  pt.amg_fplan = AmgFusePlan();
  const bool tiled = !rk && !partitioned(h) && pt.amg_kind == MFEA_PC_GAMG && nlev >= 2 &&
                     pl.l0_window != kAmgSortWindow && amg_fuse_tile_ok(pl.l0_window);
  if (tiled && amg_fuse_opted(h)) {
    const std::string ferr = build_amg_fuse(pl, amg_fuse_halo_cap(nd, pl.l0_window), pt.amg_fplan);
    if (!ferr.empty()) return fail(MFEA_EINVAL, ferr);
  }
  std::vector<int32_t> lcol2;  // the local columns, two to a word
  if (pt.amg_fplan.on) {
    lcol2.assign((pt.amg_fplan.lcol.size() + 1) / 2, 0);
    std::memcpy(lcol2.data(), pt.amg_fplan.lcol.data(), pt.amg_fplan.lcol.size() * sizeof(uint16_t));
  }
  // the level-0 label of every free row (the floating mask's scatter, launch_floating)
  std::vector<int32_t> row0_inv;
  if (!rk && nlev > 1) {
    row0_inv.assign(pl.row0.size(), -1);
    for (size_t i = 0; i < pl.row0.size(); ++i) row0_inv[pl.row0[i]] = (int32_t)i;
  }
  IndexStage ist(kAmgAlign);  // pt.amg_i's arrays: pass 1 lists their copies, stage_flush issues them
  int pass = 0;
  auto I = [&](const std::vector<int32_t>& v) -> const int32_t* {
    const size_t at = ist.put(v);
    return pass == 0 ? nullptr : pt.amg_i.ptr + at;
  };
  // (ndd, nff: the running offsets into amg_d and amg_f, pass 0's totals)
  auto carve = [&](auto* base, size_t& end, size_t n) {
    const size_t at = end;
    end += amg_al(n);
    return pass == 0 ? nullptr : base + at;
  };
  auto D = [&](size_t n) { return carve(pt.amg_d.ptr, ndd, n); };
  auto F = [&](size_t n) { return carve(pt.amg_f.ptr, nff, n); };
  // vals64: f64 values, vals32: f32 values (the numeric setup stores every
  // hierarchy value in f32 — computing in f64 — and the V-cycle reads them;
  // only A_0's symmetric blocks for the CG's w = A u stay f64)
  std::deque<std::vector<int32_t>> srows;  // built in pass 1, alive until stage_flush has run
  auto mat = [&](const SellPat& S, bool vals64, bool vals32) {
    AmgMatD m;
    m.n = S.n;
    m.npos = S.n_pos();
    for (size_t k = 0; k + 1 < S.sptr.size(); ++k) m.wmax = std::max(m.wmax, S.sptr[k + 1] - S.sptr[k]);
    m.sptr = I(S.sptr);
    const size_t nrow = S.sptr.empty() ? 0 : S.sptr.back();
    if (pass == 0) {
      ist.reserve(nrow);
    } else {
      std::vector<int32_t>& srow = srows.emplace_back(nrow, 0);  // slot row → slice
      for (size_t k = 0; k + 1 < S.sptr.size(); ++k)
        for (int32_t t = S.sptr[k]; t < S.sptr[k + 1]; ++t) srow[t] = (int32_t)k;
      m.srow = I(srow);
    }
    m.col = I(S.col);
    m.val = vals64 ? D((size_t)nb2 * m.npos) : nullptr;
    m.val32 = vals32 ? F((size_t)nb2 * m.npos) : nullptr;
    return m;
  };
  for (pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      RC(stage_begin(pt.amg_i, ist));
      HIPC(pt.amg_d.alloc(std::max<size_t>(ndd, 1)));
      HIPC(pt.amg_f.alloc(std::max<size_t>(nff, 1)));
      HIPC(hipMemsetAsync(pt.amg_d.ptr, 0, pt.amg_d.n * sizeof(double), s));
      HIPC(hipMemsetAsync(pt.amg_f.ptr, 0, pt.amg_f.n * sizeof(float), s));
      ndd = nff = 0;
    }
    pt.amg_lev.assign(nlev, AmgLevD{});
    for (int l = 0; l < nlev; ++l) {
      const AmgLevel& L = pl.lev[l];
      AmgLevD& d = pt.amg_lev[l];
      const int64_t n = L.A.n;
      const int64_t lo = rk ? rk->lo[l] : 0, hi = rk ? rk->hi[l] : n;
      d.A = mat(L.A, false, true);
      d.A.rg = row_range(L.A, lo, hi);
      if (l == 0) {  // A_0: symmetric blocks for the CG and the level-0 V-cycle kernels
        const size_t ns = (size_t)nd * (nd + 1) / 2;
        d.A.sym = D(ns * d.A.npos);
        d.A.sym32 = F(ns * d.A.npos);
      }
      d.dinv = l == 0 && nlev == 1 ? D((size_t)nb2 * n) : nullptr;  // one level: the exact block solve
      d.dinv32 = F((size_t)nb2 * n);
      d.omega = D(2);
      d.b = l ? F((size_t)nd * n) : nullptr;  // level 0 reads the CG's r
      d.x = F((size_t)nd * n);
      d.t = F((size_t)nd * n);
      d.e = l ? F((size_t)nd * n) : nullptr;  // level 0 writes the CG's u
      d.coarsest = L.coarsest ? 1 : 0;
      set_level_lanes(*h, d);
      // levels of at most this many rows run their setup on one XCD (0: never;
      // C3: levels 4-5 gain 1-2 µs per launch, level 3 at 8192 lost as much)
      constexpr int64_t kAmgX1Rows = 2048;
      d.x1 = !rk && l > 0 && n <= kAmgX1Rows ? 1 : 0;
      if (!L.coarsest) {
        d.agg = I(L.agg);
        d.P = mat(L.P, false, true);
        d.P.rg = row_range(L.P, lo, hi);
        d.pv_ptr = I(L.pv.ptr);
        d.pv_a = I(L.pv.a);
        const int64_t rlo = rk ? rk->rlo[l] : 0, rhi = rk ? rk->rhi[l] : L.R.n;
        d.R = mat(L.R, false, true);
        d.R.rg = row_range(L.R, rlo, rhi);
        d.ac_rg = row_range(pl.lev[l + 1].A, rlo, rhi);
        d.rp = I(L.rp);
        d.AP = mat(L.AP, false, false);
        d.AP.rg = row_range(L.AP, rk ? rk->aplo[l] : 0, rk ? rk->aphi[l] : L.AP.n);
        d.apval = F((size_t)nb2 * d.AP.npos);
        d.ap_ptr = I(L.ap.ptr);
        d.ap_a = I(L.ap.a);
        d.ap_b = I(L.ap.b);
        d.ac_ptr = I(L.ac.ptr);
        d.ac_a = I(L.ac.a);
        d.ac_b = I(L.ac.b);
        {  // the Galerkin product's lanes per block: its lists run 5–40 pairs (amg.hip ac_body)
          const int64_t np = std::max<int64_t>(1, pl.lev[l + 1].A.n_pos());
          const double mean = L.ac.ptr.empty() ? 0.0 : (double)L.ac.ptr.back() / (double)np;
          d.ac_lanes = mean > 24.0 ? 8 : mean > 12.0 ? 4 : mean > 6.0 ? 2 : 1;
        }
        // the compact cycle's P̃ / R̃: one partition's hierarchy, or a
        // distributed one split at level 0 only (rk->compact: level 0 on this
        // rank's P̃ / R̂ / Ã rows, the replicated levels whole; the four-step
        // distributed cycle exchanges per step instead)
        const bool cmp = !rk || (rk->compact && (l == 0 || l >= rk->n_dist));
        if (cmp && L.PT.n == n) {
          const bool own = rk && l < rk->n_dist;
          d.PT = mat(L.PT, false, true);
          d.A.at32 = F((size_t)nb2 * d.A.npos);
          d.PT.rg = own ? row_range(L.PT, rk->aplo[l], rk->aphi[l]) : row_range(L.PT, 0, n);
          d.pt_row = I(L.pt_row);
          d.pt_ap = I(L.pt_ap);
          d.pt_p = I(L.pt_p);
          d.RT = mat(L.RT, false, true);
          d.RT.rg = own ? row_range(L.RT, rk->rtlo, rk->rthi) : row_range(L.RT, 0, L.RT.n);
          d.rt_pt = I(L.rt_pt);
          d.rt_row = I(L.rt_row);
          d.compact = h->opt_amg_cycle;
        }
        if (pt.amg_coll.kc > 0 && l >= pt.amg_coll.kc) {  // the collapsed operators of this level
          const AmgCollapse::Lev& C = pt.amg_coll.lev[l - pt.amg_coll.kc];
          d.CT = mat(C.T, false, true);
          d.ct_ptr = I(C.tl.ptr);
          d.ct_a = I(C.tl.a);
          d.ct_b = I(C.tl.b);
          d.CV = mat(C.V, false, true);
          d.cv_row = I(C.vrow);
          d.cv_ptr = I(C.vl.ptr);
          d.cv_a = I(C.vl.a);
          d.cv_b = I(C.vl.b);
          d.cv_ext = I(C.va);
          d.cv_diag = I(C.vdiag);
          d.collapsed = 1;
        }
      }
    }
    pt.amg_a0_ptr = I(a0 ? a0->ptr : pl.a0.ptr);
    pt.amg_a0_a = I(a0 ? a0->a : pl.a0.a);
    pt.amg_row0_inv = !rk && nlev > 1 ? I(row0_inv) : nullptr;
    const int64_t nf = nlev ? pl.lev[0].A.n : 0;
    pt.amg_cg.n = nf;
    pt.amg_cg.lo = rk && nlev ? rk->lo[0] : 0;
    pt.amg_cg.hi = rk && nlev ? rk->hi[0] : nf;
    constexpr int kAmgWBlock = 0;  // w = A u threads per block (0: by size)
    pt.amg_cg.w_block = kAmgWBlock;
    pt.amg_cg.w_k = amg_w_k(pl);
    pt.amg_cg.cycle = h->opt_amg_cycle;
    pt.amg_cg.coll = pt.amg_coll.kc;
    pt.amg_cg.row0 = I(row0 ? *row0 : pl.row0);
    pt.amg_cg.x = D((size_t)nd * nf);
    pt.amg_cg.p = D((size_t)nd * nf);
    pt.amg_cg.s = D((size_t)nd * nf);
    pt.amg_cg.w = D((size_t)nd * nf);
    pt.amg_cg.r = D((size_t)nd * nf);
    pt.amg_cg.u = F((size_t)nd * nf);
    pt.amg_uh_stride = (int64_t)amg_al((size_t)nd * nf);
    pt.amg_uh = !rk && nlev > 1 ? F((size_t)kAmgPxSlots * pt.amg_uh_stride) : nullptr;
    pt.amg_cg.w_tile = tiled ? (int)pl.l0_window : 0;
    pt.amg_cg.skip_up0 = 0;
    pt.amg_fuse = AmgFuseD{};
    if (pt.amg_fplan.on) {
      const AmgFusePlan& fp = pt.amg_fplan;
      pt.amg_fuse.on = 1;
      pt.amg_fuse.hcap = (int)std::max<int64_t>(64, (fp.max_halo + 63) / 64 * 64);
      pt.amg_fuse.hptr = I(fp.hptr);
      pt.amg_fuse.hrow = I(fp.hrow);
      pt.amg_fuse.hpt = I(fp.hpt);
      pt.amg_fuse.lcol = reinterpret_cast<const int16_t*>(I(lcol2));
    }
    // the merged levels' operators, lists and vector buffer
    pt.amg_mg = AmgMergeD{};
    if (pt.amg_mplan.on) {
      const AmgMerge& M = pt.amg_mplan;
      AmgMergeD& g = pt.amg_mg;
      g.n1 = M.n1;
      g.n2 = M.n2;
      g.DQ = mat(M.DQ, false, true);
      g.DQ.rg = row_range(M.DQ, 0, M.DQ.n);
      g.U = mat(M.U, false, true);
      g.U.rg = row_range(M.U, 0, M.U.n);
      g.dq_dst = I(M.dq_dst);
      g.dq_split = M.dq_split;
      g.dq_ext = I(M.dq_ext);
      g.dq_ptr = I(M.dq_l.ptr);
      g.dq_a = I(M.dq_l.a);
      g.dq_b = I(M.dq_l.b);
      g.u_ext = I(M.u_ext);
      g.u_ptr = I(M.u_l.ptr);
      g.u_a = I(M.u_l.a);
      g.u_b = I(M.u_l.b);
      g.B = F((size_t)nd * (M.n1 + 2 * M.n2 + 1));
    }
  }
  RC(stage_flush(h, pt.amg_i, ist));
  pt.amg_x2 = nlev > 2 ? pt.amg_lev[2].x : nullptr;
  pt.amg_e2 = nlev > 2 ? pt.amg_lev[2].e : nullptr;
  set_merge(h, pt);
  {
    std::vector<int64_t> rows(nlev);
    for (int l = 0; l < nlev; ++l) rows[l] = pl.lev[l].A.n;
    // the single-workgroup tail holds whole levels: never a split one
    const int first = rk ? std::max(1, rk->n_dist) : 1;
    pt.amg_tail = first < nlev ? amg_tail_level(rows.data() + first - 1, nlev - first + 1, h->opt_amg_tail_rows) : 0;
    if (pt.amg_tail > 0) pt.amg_tail += first - 1;
    pt.amg_first = first;
  }
  if (!rk && nlev > 1) {  // the floating-row mask (zero until ensure_amg fills it)
    HIPC(pt.amg_fmask.alloc(std::max<int64_t>(pl.lev[0].A.n, 1)));
    HIPC(hipMemsetAsync(pt.amg_fmask.ptr, 0, pt.amg_fmask.n, s));
    pt.amg_lev[0].fmask = pt.amg_fmask.ptr;
  }
  // the smoothing weights (ρ̂ per level in place of the Gershgorin estimate)
  pt.amg_om_own = !rk;
  pt.amg_om_spatial = pl.spatial;
  HIPC(pt.amg_levd.alloc(std::max(nlev, 1)));
  return apply_coarse_omega(h, pt);
}

// The element activity of the handle's single partition, on the host.
int current_active(mfea_handle* h, Part& pt) {
  if (h->act_host_ok && h->act_host.size() == (size_t)pt.P.n_elems) return 0;
  h->act_host.resize(pt.P.n_elems);
  if (pt.P.n_elems)
    HIPC(hmemcpy(h, h->act_host.data(), pt.active.ptr, pt.P.n_elems, hipMemcpyDeviceToHost));
  h->act_count = (int64_t)std::count(h->act_host.begin(), h->act_host.end(), (uint8_t)1);
  h->act_host_ok = true;
  return 0;
}

// Partitioned GAMG: the halo plan (ghost couplings, u send rows) for the
// plan's active set, uploaded next to the hierarchy.
int upload_amg_halo(mfea_handle* h, Part& pt, const std::vector<uint8_t>& key) {
  const PartPlan& pl = pt.plan;
  const Pattern& P = pt.P;
  std::vector<int32_t> xs(pl.xsend_node.size()), xr(pl.xrecv_node.size());
  for (size_t i = 0; i < xs.size(); ++i) xs[i] = P.iperm[pl.xsend_node[i]];
  for (size_t i = 0; i < xr.size(); ++i) xr[i] = P.iperm[pl.xrecv_node[i]];
  const std::string err = build_amg_halo(P, key, pt.amg, xs, xr, pt.amg_halo);
  if (!err.empty()) return fail(MFEA_EINVAL, "AMG halo: " + err);
  const AmgHalo& hl = pt.amg_halo;
  const int nd = pt.amg.nd;
  hipStream_t s = h->stream;
  HIPC(pt.amg_hd.alloc(nd * (xs.size() + xr.size()) + 1));
  HIPC(hipMemsetAsync(pt.amg_hd.ptr, 0, pt.amg_hd.n * sizeof(double), s));
  IndexStage st;
  size_t send_rows = 0, gptr = 0, gslot = 0, grecv = 0;
  for (int pass = 0; pass < 2; ++pass) {  // count, then fill
    if (pass == 1) RC(stage_begin(pt.amg_hi, st));
    send_rows = st.put(hl.send_rows);
    gptr = st.put(hl.gptr);
    gslot = st.put(hl.gslot);
    grecv = st.put(hl.grecv);
    st.reserve(1);  // (an empty last list still points inside)
  }
  RC(stage_flush(h, pt.amg_hi, st));
  const int32_t* ib = pt.amg_hi.ptr;
  AmgDist& d = pt.amg_dist;
  d = AmgDist{};
  d.rank = pt.rank;
  d.gall[0] = pt.dv.gall[0];
  d.gall[1] = pt.dv.gall[1];
  d.gsend = pt.dv.gsend;
  d.zero_w = h->world > 1 && h->opt_dist_sums == 1 ? h->world : 0;
  d.send_rows = ib + send_rows;
  d.n_send = (int64_t)hl.send_rows.size();
  d.gptr = ib + gptr;
  d.gslot = ib + gslot;
  d.grecv = ib + grecv;
  d.sval = pt.val.ptr;
  d.G = pt.G;
  d.usend = pt.amg_hd.ptr;
  d.urecv = pt.amg_hd.ptr + nd * xs.size();
  return 0;
}

// The floating-row mask of the device's current activity in level-0 labels
// (one partition's own hierarchy: a partition cannot tell alone what is
// floating): connected components on the device (kernels.hpp
// launch_floating), four launches on the stream, no host pass or wait
int enqueue_fmask(mfea_handle* h, Part& pt) {
  const Pattern& P = pt.P;
  if (P.n_free == 0 || !pt.amg_row0_inv) return 0;
  ++pt.fmask_gen;
  HIPC(pt.cc_parent.alloc(std::max<int64_t>(P.n_nodes, 1)));
  HIPC(pt.cc_anch.alloc(std::max<int64_t>(P.n_nodes, 1)));
  launch_floating(h->stream, P.n_nodes, P.n_free, P.n_nodes - P.n_ghost, pt.slice_ptr.ptr, pt.row_len.ptr,
                  pt.s_col.ptr, pt.s_elem.ptr, pt.active.ptr, pt.cc_parent.ptr, pt.cc_anch.ptr, pt.amg_row0_inv,
                  pt.amg_fmask.ptr, h->opt_cc_tile);
  HIPC(hipGetLastError());
  return 0;
}

// the multicolour sweep's arrays for a one-level plan (MFEA_PC_SOR / _ICC);
// a GAMG plan: none (amg_cg.sweep = 0)
int upload_sweep(mfea_handle* h, Part& pt, int kind) {
  pt.swd = SweepD{};
  pt.amg_cg.sweep = 0;
  if (kind != MFEA_PC_SOR && kind != MFEA_PC_ICC) return 0;
  const SweepPlan& sp = pt.sweep;
  if (sp.colors > kSweepMaxColors) return fail(MFEA_EINVAL, "sweep plan: too many colours");
  const int nd = pt.amg.nd, nb2 = nd * nd, ns = nd * (nd + 1) / 2;
  const int64_t ne = sp.n_entries();
  const size_t nlo = sp.lo_ent.size(), nup = sp.up_ent.size();
  HIPC(pt.sw_f.alloc((size_t)ne * (nb2 + ns) + (nlo + nup) * nb2 + 1));
  HIPC(pt.sw_y.alloc((size_t)ne * nd + 1));
  hipStream_t s = h->stream;
  // pads and first steps are never written by the setup: zero them once
  HIPC(hipMemsetAsync(pt.sw_f.ptr, 0, pt.sw_f.n * sizeof(float), s));
  HIPC(hipMemsetAsync(pt.sw_y.ptr, 0, pt.sw_y.n * sizeof(double), s));
  SweepD& w = pt.swd;
  // the index arrays and their pointers, one after the other in sw_i
  struct Arr {
    const std::vector<int32_t>* v;
    const int32_t** d;
  };
  const Arr arr[] = {{&sp.wsteps, &w.wsteps}, {&sp.row, &w.row},       {&sp.ppos, &w.ppos},     {&sp.dpos, &w.dpos},
                     {&sp.lo_ptr, &w.lo_ptr}, {&sp.lo_ent, &w.lo_ent}, {&sp.lo_pos, &w.lo_pos}, {&sp.up_ptr, &w.up_ptr},
                     {&sp.up_ent, &w.up_ent}, {&sp.up_pos, &w.up_pos}};
  IndexStage st;
  for (int pass = 0; pass < 2; ++pass) {  // count, then fill
    if (pass == 1) RC(stage_begin(pt.sw_i, st));
    for (const Arr& a : arr) {
      const size_t at = st.put(*a.v);
      if (pass == 1) *a.d = pt.sw_i.ptr + at;
    }
    st.reserve(1);  // (an empty last list still points inside)
  }
  RC(stage_flush(h, pt.sw_i, st));
  w.n = sp.n;
  w.ne = ne;
  w.colors = sp.colors;
  w.dic = kind == MFEA_PC_ICC ? 1 : 0;
  for (int c = 0; c <= sp.colors; ++c) w.cw[c] = sp.cwave[c];
  float* fp = pt.sw_f.ptr;
  w.pv = fp;
  w.dt = fp + (size_t)ne * nb2;
  w.lov = w.dt + (size_t)ne * ns;
  w.upv = w.lov + nlo * nb2;
  w.y = pt.sw_y.ptr;
  pt.amg_cg.sweep = 1;
  return 0;
}

// the preconditioner application u = M r of one PCG iteration (gate: its
// flag; NULL: ungated)
// (cg: pt.amg_cg with another u, the lazy p, x chain's slot — px_cg)
void launch_precond(mfea_handle* h, Part& pt, const int32_t* gate, const AmgCg* cg) {
  const AmgCg& c = cg ? *cg : pt.amg_cg;
  if (pt.amg_cg.sweep) launch_sweep(h->stream, pt.amg.nd, pt.swd, c, gate);
  else launch_amg_vcycle(h->stream, pt.amg.nd, pt.amg_lev.data(), (int)pt.amg_lev.size(), c, pt.amg_tail, gate,
                         0, pt.amg_mg.on ? &pt.amg_mg : nullptr);
}

// The lazy p, x chain (option amg_lazy_px, amg_kernels.hpp AmgPx): the
// one-partition GAMG solve whose level 0 forms its x in the update
bool amg_lazy(const mfea_handle* h, const Part& pt) {
  return h->opt_amg_lazy_px && pt.amg_uh && !pt.amg_cg.sweep && !pt.amg_lev.empty() && !pt.amg_lev[0].coarsest;
}
// the CG's arrays with update k's slot as u: what its V-cycle writes and its
// w = A u reads (a host constant of each launch)
AmgCg px_cg(const Part& pt, int k) {
  AmgCg c = pt.amg_cg;
  c.u = pt.amg_uh + (int64_t)amg_px_slot(k) * pt.amg_uh_stride;
  return c;
}
AmgPx px_of(const Part& pt, int k0, int cnt) {
  AmgPx px;
  px.uh = pt.amg_uh;
  px.stride = pt.amg_uh_stride;
  px.k0 = k0;
  px.cnt = cnt;
  return px;
}
// Level 0's up sweep and w = A u as one launch (k_amg_up_w): the plan's halo
// fits (upload_amg) and the cycle run now is the compact, unmerged one with
// one lane per P̃_0 row — the merged cycle, the four-step cycle, the sweeps
// and the partitioned solves keep their launches
bool amg_fused(const mfea_handle* h, const Part& pt) {
  return amg_fuse_opted(h) && pt.amg_fuse.on && pt.amg_cg.w_tile > 0 && !pt.amg_cg.sweep && !pt.amg_mg.on &&
         pt.amg_cg.cycle == 1 && amg_compact_ok(pt.amg_lev.data(), (int)pt.amg_lev.size(), 0) &&
         amg_up_lanes(pt.amg_lev[0]) == 1;
}
// the V-cycle up to level 0's up sweep, then that sweep and w = A u; or the
// V-cycle and w = A u
void launch_vcycle_w(mfea_handle* h, Part& pt, int j, bool first, const AmgCg& cg) {
  hipStream_t s = h->stream;
  if (amg_fused(h, pt)) {
    AmgCg c = cg;
    c.skip_up0 = 1;
    launch_precond(h, pt, nullptr, &c);
    launch_amg_up_w(s, pt.amg.nd, j, first, pt.amg_lev[0], pt.amg_lev[1], cg, pt.amg_fuse, pt.slots.ptr,
                    pt.cg_part.ptr);
  } else {
    launch_precond(h, pt, nullptr, &cg);
    launch_amg_cg_w(s, pt.amg.nd, j, first, pt.amg_lev[0], cg, pt.slots.ptr, pt.cg_part.ptr);
  }
}
// replay launches of a chunk of `chunk` groups (enqueue_amg_chunk)
int px_replays(int chunk) { return 1 + (chunk > 0 ? (chunk - 1) / (kAmgPxSlots - 1) : 0); }

// (Re)build the hierarchy when the active set differs from the plan's.  One
// partition: the host view of the activity (downloaded only when a post
// kernel changed it); partitioned: each partition's own elements, read back.
int upload_sweep(mfea_handle* h, Part& pt, int kind);

// every element active in `a` is active in `b`: a hierarchy built for b is
// kept for a only then — A_0's slot lists hold b's elements alone, so an
// element that came back since would be missing from the CG's w = A u
// (its couplings absent while the diagonal has them)
static bool active_subset(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
  if (a.size() != b.size()) return false;
  for (size_t e = 0; e < a.size(); ++e)
    if (a[e] && !b[e]) return false;
  return true;
}

// the chain-piece plan with at most kSweepMaxColors colours: shorter pieces
// (fewer couplings per piece) until it fits — pieces of one row are a point
// colouring, max degree + 1 colours at most
std::string build_sweep_bounded(const AmgPlan& plan, int piece_len, SweepPlan& sp) {
  for (int m = piece_len;; m = std::max(1, m / 2)) {
    const std::string err = build_sweep(plan, m, sp);
    if (!err.empty() || sp.colors <= kSweepMaxColors) return err;
    if (m == 1) return "sweep plan: more than 32 colours";
  }
}

int ensure_amg(mfea_handle* h, Part& pt, bool* rebuilt, int kind = MFEA_PC_GAMG) {
  *rebuilt = false;
  if (pt.amg_ok && pt.amg_kind != kind) {  // another preconditioner's plan
    pt.amg_ok = false;
    pt.amg_last_iters = 0;
  }
  const bool dm = partitioned(h);
  // no activity change since the plan / mask last matched it: nothing to do
  // (no O(E) key compares on the hot path)
  if (!dm && pt.amg_ok && !pt.amg_stale && pt.amg_seen_gen == h->act_gen) return 0;
  // the activity moved only by failures since the plan's key was set (post
  // kept the host activity current from the failed ids): keep the hierarchy
  // with no host O(E) pass — the floating mask is recomputed on the device
  if (!dm && pt.amg_ok && !pt.amg_stale && h->opt_amg_reuse && pt.amg_lev.size() > 1 && h->act_host_ok &&
      pt.amg_sub_gen == h->act_sub_gen) {
    RC(enqueue_fmask(h, pt));
    pt.amg_reused = h->act_count != pt.amg_key_count;
    pt.amg_seen_gen = h->act_gen;
    return 0;
  }
  std::vector<uint8_t> local;
  if (dm) {
    local.resize(pt.P.n_elems);
    if (pt.P.n_elems) HIPC(hmemcpy(h, local.data(), pt.active.ptr, pt.P.n_elems, hipMemcpyDeviceToHost));
  } else {
    RC(current_active(h, pt));
  }
  const std::vector<uint8_t>& key = dm ? local : h->act_host;
  pt.amg_reused = false;
  if (!dm && pt.amg_ok && pt.amg_lev.size() > 1 &&
      (pt.amg_key == key || (h->opt_amg_reuse && !pt.amg_stale && active_subset(key, pt.amg_key)))) {
    // keep the hierarchy: the numeric setup re-forms its values from the new
    // K (failed elements are zero slots); only pieces cut off from both grips
    // need care — their P_0 rows are zeroed so they stay exactly at zero
    RC(enqueue_fmask(h, pt));
    pt.amg_reused = pt.amg_key != key;
    pt.amg_seen_gen = h->act_gen;
    pt.amg_sub_gen = h->act_sub_gen;  // key ⊆ amg_key, compared
    return 0;
  }
  if (pt.amg_ok && pt.amg_key == key) {
    if (!dm) pt.amg_seen_gen = h->act_gen;
    if (!dm || pt.dev_plan == 0) return 0;
    RC(drain_before_upload(h, "plan upload"));
    destroy_graph(h);  // the device holds the global plan: upload this one again
    RC(upload_amg(h, pt, pt.amg));
    RC(upload_amg_halo(h, pt, key));
    pt.dev_plan = 0;
    ++pt.amg_gen;
    return 0;
  }
  pt.amg_ok = false;
  HostLap clk;
  const auto build_t0 = std::chrono::steady_clock::now();
  AmgLayout lay;
  lay.spatial = h->opt_amg_spatial;
  lay.by_a = h->opt_amg_cycle == 1;
  lay.l0_window = amg_l0_window(h, pt, kind);
  const bool sweep = kind == MFEA_PC_SOR || kind == MFEA_PC_ICC;
  std::string err = build_amg(pt.P, key, lane_dofs(h), pt.amg, sweep ? 1 : h->opt_amg_max_levels, nullptr,
                              amg_strength(h), lay);
  if (err.empty() && sweep) err = build_sweep_bounded(pt.amg, h->opt_sweep_piece, pt.sweep);
  if (!err.empty()) return fail(MFEA_EINVAL, "AMG setup: " + err);
  clk.lap("plan build");
  RC(drain_before_upload(h, "plan upload"));
  clk.lap("drain");
  destroy_graph(h);
  pt.amg_kind = kind;
  RC(upload_amg(h, pt, pt.amg));
  RC(upload_sweep(h, pt, kind));
  if (dm) RC(upload_amg_halo(h, pt, key));
  clk.lap("plan upload");
  pt.dev_plan = 0;
  pt.amg_key = key;
  pt.amg_ok = true;
  pt.amg_stale = false;
  pt.amg_build_iters = -1;
  pt.amg_excess_s = 0.0;
  pt.amg_build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - build_t0).count();
  pt.amg_reused = false;
  if (!dm && pt.amg_lev.size() > 1) RC(enqueue_fmask(h, pt));
  clk.lap("floating mask");
  if (!dm) pt.amg_seen_gen = h->act_gen;
  pt.amg_sub_gen = dm ? -1 : h->act_sub_gen;
  pt.amg_key_count = (int64_t)std::count(key.begin(), key.end(), (uint8_t)1);
  ++pt.amg_gen;
  *rebuilt = true;
  return 0;
}

void enqueue_amg_iteration(mfea_handle* h, Part& pt, int j, bool profile) {
  hipStream_t s = h->stream;
  const int nd = pt.amg.nd;
  const AmgLevD& L0 = pt.amg_lev[0];
  // (the default form: the slim update, u in its slot — the replay, once a
  // chunk, is not part of an iteration)
  const bool lazy = amg_lazy(h, pt);
  const AmgCg cg = lazy ? px_cg(pt, j) : pt.amg_cg;
  launch_amg_cg_update(s, nd, j, L0, cg, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr, nullptr, lazy);
  launch_vcycle_w(h, pt, j, profile, cg);
}

// ---- partitioned GAMG exchanges -------------------------------------------
// u of the send rows → the peers' urecv (the displacement-halo plan, ND
// doubles per node)
int xchg_u(mfea_handle* h) {
  hipStream_t s = h->stream;
  const int64_t nd = part0(h).amg.nd;
  if (h->world > 1) {
    Part& pt = part0(h);
    const PartPlan& pl = pt.plan;
    if (pl.xpeers.empty()) return 0;
    NCCLC(ncclGroupStart());
    for (size_t i = 0; i < pl.xpeers.size(); ++i) {
      if (pl.xsend_cnt[i])
        NCCLC(ncclSend(pt.amg_dist.usend + nd * pl.xsend_off[i], (size_t)(nd * pl.xsend_cnt[i]), ncclFloat64,
                       pl.xpeers[i], h->comm, s));
      if (pl.xrecv_cnt[i])
        NCCLC(ncclRecv(const_cast<double*>(pt.amg_dist.urecv) + nd * pl.xrecv_off[i],
                       (size_t)(nd * pl.xrecv_cnt[i]), ncclFloat64, pl.xpeers[i], h->comm, s));
    }
    NCCLC(ncclGroupEnd());
    return 0;
  }
  for (auto& a : h->parts) {
    const PartPlan& pa = a->plan;
    for (size_t i = 0; i < pa.xpeers.size(); ++i) {
      if (!pa.xsend_cnt[i]) continue;
      Part& b = *h->parts[pa.xpeers[i]];
      const PartPlan& pb = b.plan;
      const auto it = std::lower_bound(pb.xpeers.begin(), pb.xpeers.end(), a->rank);
      const size_t jb = (size_t)(it - pb.xpeers.begin());
      if (it == pb.xpeers.end() || *it != a->rank || pb.xrecv_cnt[jb] != pa.xsend_cnt[i])
        return fail(MFEA_EINVAL, "internal: asymmetric u halo");
      HIPC(hipMemcpyAsync(const_cast<double*>(b.amg_dist.urecv) + nd * pb.xrecv_off[jb],
                          a->amg_dist.usend + nd * pa.xsend_off[i], nd * pa.xsend_cnt[i] * sizeof(double),
                          hipMemcpyDeviceToDevice, s));
    }
  }
  return 0;
}

// every rank's 4 partial sums (gsend) → row `rank` of every rank's gall[q]
int xchg_sums(mfea_handle* h, int q) {
  hipStream_t s = h->stream;
  if (h->world > 1 && h->opt_dist_sums == 1) {  // one all-reduce: every row but the own zeroed (k_amg_gsum)
    Part& pt = part0(h);
    NCCLC(ncclAllReduce(pt.dv.gall[q], pt.dv.gall[q], (size_t)4 * h->world, ncclFloat64, ncclSum, h->comm, s));
    return 0;
  }
  if (h->world > 1) {
    Part& pt = part0(h);
    NCCLC(ncclGroupStart());
    RC(sums_p2p(h, pt.dv.gsend, pt.dv.gall[q]));
    NCCLC(ncclGroupEnd());
    return 0;
  }
  GallCopy g;  // partitions on one device: one launch for every pair
  for (auto& a : h->parts) {
    if (g.n == 64) return fail(MFEA_EINVAL, "internal: more than 64 partitions");
    g.gsend[g.n] = a->dv.gsend;
    g.gall[g.n] = a->dv.gall[q];
    g.rank[g.n] = a->rank;
    ++g.n;
  }
  launch_gall_copy(s, g);
  HIPC(hipGetLastError());
  return 0;
}

// one partitioned GAMG iteration j on every partition: update (gathered sums)
// → local V-cycle → u halo → w = A u with the ghost couplings → this rank's
// sums → all-gather.  Two exchanges per iteration (the V-cycle output is not
// computable from a neighbour's state, unlike the Jacobi lanes' records).
int enqueue_amg_dist_iteration(mfea_handle* h, int j) {
  hipStream_t s = h->stream;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int nd = pt.amg.nd;
    launch_amg_cg_update(s, nd, j, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr,
                         &pt.amg_dist);
    launch_amg_vcycle(s, nd, pt.amg_lev.data(), (int)pt.amg_lev.size(), pt.amg_cg, pt.amg_tail, nullptr);
    launch_amg_pack_u(s, nd, pt.amg_cg, pt.amg_dist);
  }
  HIPC(hipGetLastError());
  RC(xchg_u(h));
  const int q = (j & 1) ^ 1;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_w(s, pt.amg.nd, j, false, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr,
                    &pt.amg_dist);
    launch_amg_gsum(s, pt.amg_cg, cg_part_buf(pt, q), pt.amg_dist, q);
  }
  HIPC(hipGetLastError());
  return xchg_sums(h, q);
}

int enqueue_amg_dist_chunk(mfea_handle* h, int chunk) {
  for (int j = 0; j < chunk; ++j) RC(enqueue_amg_dist_iteration(h, j));
  for (auto& pp : h->parts) launch_cg_advance(h->stream, chunk, pp->slots.ptr, pp->state.ptr, pp->mirror);
  HIPC(hipGetLastError());
  return 0;
}

// One replayed chunk = `chunk` groups of (V-cycle j, w_j, update j+1): the
// chunk ENDS with an update, so the last planned chunk leaves the device
// knowing whether the solve converged and no chunk of early-exiting launches
// is queued after the converging update (each gated launch still costs
// ≈ 4 µs).  update 0 runs before the first chunk (solve_amg).
//
// close (solve_amg's amg_close): the chunk ends … update, k_amg_rnorm,
// advance.  The chunk's last update has moved r and only the NEXT update
// would test it, behind a V-cycle and a w = A u that nothing else needs when
// it has converged: the advance kernel tests ‖r‖² from k_amg_rnorm's partials
// instead (k_cg_advance's closing form), so a planned batch of iters − 1
// groups ends the solve — iters V-cycles in all, not iters + 1.  chunk may
// then be 0: the entry's update 0, the closing check, nothing else.
void enqueue_amg_chunk(mfea_handle* h, Part& pt, int chunk, bool close) {
  hipStream_t s = h->stream;
  const int nd = pt.amg.nd;
  const AmgLevD& L0 = pt.amg_lev[0];
  // The preconditioner and w = A u launches carry no gate: once the update
  // kernel stops the solve (converged, max_it, breakdown) it leaves x, r, p,
  // s and level 0's x unchanged, and every later V-cycle / sweep / w launch
  // is a pure function of those — it rewrites the values it wrote before.  A
  // gate flag cost each launch a load from another XCD's L2 ahead of its
  // first wait (vector loads complete in order), ≈ 1 µs per launch.
  //
  // The lazy p, x chain (amg_lazy_px): the V-cycle of update k writes its u
  // to slot amg_px_slot(k), so past the stop the chunk's remaining V-cycles
  // write those same values into later slots instead of one buffer.  The
  // replay reads only the slots of updates whose record says they ran, and
  // every update past the stop records kStop: harmless.  The replay sits
  // behind the chunk's last update — in the closing check's launch, else a
  // launch of its own — and before the advance rolls the records over; a
  // chunk longer than the slots replays whenever they are full.  k0: the
  // first update not yet replayed (update 0 is the entry's; in a later chunk
  // slots[1] is the rolled-over record, which the replay skips).
  const bool lazy = amg_lazy(h, pt);
  int k0 = 0;
  for (int j = 0; j < chunk; ++j) {
    const AmgCg cg = lazy ? px_cg(pt, j + 1) : pt.amg_cg;
    launch_vcycle_w(h, pt, j, false, cg);
    launch_amg_cg_update(s, nd, j + 1, L0, cg, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr, nullptr, lazy);
    if (lazy && (j + 1) % (kAmgPxSlots - 1) == 0 && j + 1 < chunk) {
      launch_amg_px_replay(s, nd, pt.amg_cg, pt.slots.ptr, px_of(pt, k0, j + 2 - k0));
      k0 = j + 2;
    }
  }
  if (lazy && close) launch_amg_rnorm_px(s, nd, pt.amg_cg, cg_part_buf(pt, 2), pt.slots.ptr, px_of(pt, k0, chunk + 1 - k0));
  else if (lazy) launch_amg_px_replay(s, nd, pt.amg_cg, pt.slots.ptr, px_of(pt, k0, chunk + 1 - k0));
  else if (close) launch_amg_rnorm(s, nd, pt.amg_cg, cg_part_buf(pt, 2));
  launch_cg_advance(s, chunk, pt.slots.ptr, pt.state.ptr, pt.mirror, 1, close ? cg_part_buf(pt, 2) : nullptr,
                    close ? (int)amg_w_grid(pt.amg_cg) : 0);
}

// hierarchy values for the current K (the per-solve numeric setup)
void enqueue_amg_setup(mfea_handle* h, Part& pt, double reg) {
  hipStream_t s = h->stream;
  const int nd = pt.amg.nd, nlev = (int)pt.amg_lev.size();
  const bool compact = pt.amg_cg.cycle == 1 && nlev > 1 && pt.amg_lev[0].compact;
  const bool fused = compact && h->opt_amg_fuse_setup && !pt.amg_cg.sweep;
  launch_amg_a0(s, nd, pt.amg_lev[0], sell_op(pt), pt.amg_cg.row0, pt.amg_a0_ptr, pt.amg_a0_a, reg,
                fused && pt.amg_lev[0].a0full);
  if (pt.amg_cg.sweep) {
    launch_sweep_setup(s, nd, pt.swd, pt.amg_lev[0]);
    return;
  }
  bool merged_done = false;
  if (fused) {
    merged_done = launch_amg_setup_fused(s, nd, pt.amg_lev.data(), nlev, pt.amg_cg.coll, &pt.amg_mg);
  } else {
    for (int l = 0; l < nlev; ++l)
      launch_amg_level_setup(s, nd, pt.amg_lev[l], l + 1 < nlev ? &pt.amg_lev[l + 1] : nullptr, l == 0);
    launch_amg_compact_setup(s, nd, pt.amg_lev.data(), nlev, compact ? pt.amg_cg.coll : 0);
  }
  if (pt.amg_mg.on && !merged_done) launch_amg_merge_setup(s, nd, pt.amg_lev.data(), pt.amg_mg);
}

// FNV-1a over 8-byte words (then the tail bytes): the setup graph's key is
// hashed on every solve while the GPU runs the assembly, over ≈ 10 KB of level
// views — byte by byte that host work outlasted C2's assembly
uint64_t fnv1a(uint64_t k, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    std::memcpy(&w, b + i, 8);
    k = (k ^ w) * 1099511628211ULL;
  }
  for (; i < n; ++i) k = (k ^ b[i]) * 1099511628211ULL;
  return k;
}

int enqueue_post_work(mfea_handle* h, double max_strain);

// The solve's entry behind the setup: level-0 b from the CG's r, the first
// preconditioner application, w = A u, update 0 (solve_amg)
// (skip_init: k_amg_start has done launch_amg_cg_init's work, solve_amg)
void enqueue_amg_entry(mfea_handle* h, Part& pt, bool skip_init = false) {
  hipStream_t s = h->stream;
  const int nd = pt.amg.nd;
  const AmgLevD& L0 = pt.amg_lev[0];
  if (!skip_init) launch_amg_cg_init(s, nd, L0, pt.amg_cg, cg_vecs(pt).r[0]);
  const bool lazy = amg_lazy(h, pt);  // (update 0's u in slot 0: the first chunk's replay applies it)
  const AmgCg cg = lazy ? px_cg(pt, 0) : pt.amg_cg;
  launch_vcycle_w(h, pt, 0, true, cg);
  launch_amg_cg_update(s, nd, 0, L0, cg, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr, nullptr, lazy);  // update 0
}

// The fused RHS of the row gather (kernels.hpp AsmRhs) on pt's vectors: the
// amplitudes dy[0..1] by value, or (dy NULL) read from the device pair dyp
static AsmRhs asm_rhs(const mfea_handle* h, Part& pt, const double* dy, const double* dyp) {
  const Pattern& P = pt.P;
  const BcForm bc = h->bc.form(pt);
  AsmRhs q{};
  q.code = pt.code.ptr;
  q.top_end = P.n_free + P.n_top;
  q.bot_end = P.n_nodes - P.n_ghost;
  if (dy) {
    q.dy_top = dy[0];
    q.dy_bot = dy[1];
  }
  q.dyp = dyp;
  q.grip = h->bc.grip;
  q.vec = bc.grip != nullptr;
  q.field = bc.field;
  if (bc.load) q.load = *bc.load;
  q.nf = P.n_free;
  q.r = pt.r.ptr;
  q.x = pt.x.ptr;
  q.partials = pt.partials.ptr;
  q.ticket = tix(pt, 0);
  q.red_out = pt.red.ptr;
  return q;
}

// mfea_step's deferred assembly (option step_graph) at the head of the setup
// graph: the grip displacements from pinned h_red[14..15] (a copy node, read
// at replay), the row gather with the fused RHS reading them from d_dy, the
// CG start — k_assemble<true> / k_cg_init_finalize exactly as eager
void enqueue_step_head(mfea_handle* h, Part& pt, const mfea_solve_opts* o) {
  hipStream_t s = h->stream;
  const Pattern& P = pt.P;
  (void)hipMemcpyAsync(h->d_dy.ptr, h->h_red + 14, 2 * sizeof(double), hipMemcpyHostToDevice, s);
  const AsmRhs q = asm_rhs(h, pt, nullptr, h->d_dy.ptr);
  launch_assemble(s, P.n_nodes, pt.xyz_d.ptr, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr, pt.s_elem.ptr,
                  pt.active.ptr, h->mat, pt.G, pt.val.ptr, pt.diag.ptr, &q, h->sec_d());
  launch_cg_init_finalize(s, pt.red.ptr, o->rtol, o->atol, o->norm, o->max_it, o->reg, pt.state.ptr,
                          pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
}

// The numeric setup replayed as one captured graph (single partition): the
// eager launches cost the host ≈ 5–8 µs each (kernel arguments of 1.5–3 KB),
// more than the GPU spends on the deep levels' kernels; recaptured whenever
// anything the launches read changes (the key hashes all of it).  entry: the
// solve's entry launches captured behind the setup (no phase event between
// them); head (non-null): mfea_step's assembly and CG start before it
// everything enqueue_amg_setup's launches take but K's values and the
// floating mask's: the level views, the level-0 operator, the options, reg
uint64_t amg_setup_key(mfea_handle* h, Part& pt, double reg) {
  uint64_t k = 1469598103934665603ULL;
  k = fnv1a(k, pt.amg_lev.data(), pt.amg_lev.size() * sizeof(AmgLevD));
  k = fnv1a(k, &pt.amg_mg, sizeof pt.amg_mg);
  const SellOp op = sell_op(pt);
  k = fnv1a(k, &op, sizeof op);
  const void* ptrs[4] = {pt.amg_cg.row0, pt.amg_a0_ptr, pt.amg_a0_a, pt.amg_levd.ptr};
  k = fnv1a(k, ptrs, sizeof ptrs);
  const int ints[5] = {pt.amg.nd, h->opt_amg_fuse_setup, pt.amg_cg.cycle, pt.amg_cg.coll, pt.amg_cg.sweep};
  k = fnv1a(k, &pt.swd, sizeof pt.swd);
  k = fnv1a(k, ints, sizeof ints);
  // (the entry's launches: fused or not, the tiles, the halo plan's arrays)
  const int64_t fz[3] = {amg_fused(h, pt) ? 1 : 0, pt.amg_cg.w_tile, pt.amg_fuse.hcap};
  const void* fptrs[4] = {pt.amg_fuse.hptr, pt.amg_fuse.hrow, pt.amg_fuse.hpt, pt.amg_fuse.lcol};
  k = fnv1a(k, fz, sizeof fz);
  k = fnv1a(k, fptrs, sizeof fptrs);
  k = fnv1a(k, &reg, sizeof reg);
  return k;
}

// k0: amg_setup_key of these arguments.  keep: the hierarchy's values are
// current (solve_amg) — the graph without the setup's launches, cached beside
// the one with them; nothing at all where no head / entry / tail rides along
int launch_amg_setup_graph(mfea_handle* h, Part& pt, double reg, uint64_t k0, bool keep, bool entry = false,
                           const mfea_solve_opts* head = nullptr, const mfea_solve_opts* start = nullptr,
                           int tail = -1, int tag = 0, bool close = false, bool skip_init = false) {
  hipStream_t s = h->stream;
  uint64_t k = k0;
  const int form = keep ? 1 : 0;
  k = fnv1a(k, &form, sizeof form);
  if (keep && !entry && !head && !start && tail < 0) return 0;
  if (entry) {
    const CgVecs v = cg_vecs(pt);
    const void* eptrs[4] = {v.r[0], pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr};
    k = fnv1a(k, eptrs, sizeof eptrs);
    k = fnv1a(k, &pt.amg_cg, sizeof pt.amg_cg);
    k = fnv1a(k, &pt.amg_kind, sizeof pt.amg_kind);
    const int si = skip_init ? 1 : 0;
    k = fnv1a(k, &si, sizeof si);
    const int lz = amg_lazy(h, pt) ? 1 : 0;
    k = fnv1a(k, &lz, sizeof lz);
    k = fnv1a(k, &pt.amg_uh, sizeof pt.amg_uh);
  }
  if (start) {  // the CG start (k_cg_init_finalize) at the graph's head
    const double sd[3] = {start->rtol, start->atol, start->reg};
    const int si[2] = {start->norm, start->max_it};
    const void* sp[3] = {pt.red.ptr, pt.state.ptr, pt.cg_part.ptr};
    k = fnv1a(k ^ 0x5a5a, sd, sizeof sd);
    k = fnv1a(k, si, sizeof si);
    k = fnv1a(k, sp, sizeof sp);
  }
  if (head) {
    const void* hptrs[10] = {pt.xyz_d.ptr, pt.s_elem.ptr, pt.active.ptr, pt.code.ptr, pt.r.ptr,
                             pt.x.ptr, pt.partials.ptr, pt.red.ptr, h->d_dy.ptr, h->h_red};
    k = fnv1a(k, hptrs, sizeof hptrs);
    const double hd[3] = {head->rtol, head->atol, head->reg};
    const int hi[2] = {head->norm, head->max_it};
    k = fnv1a(k, hd, sizeof hd);
    k = fnv1a(k, hi, sizeof hi);
    k = fnv1a(k, &h->mat, sizeof h->mat);
    k = fnv1a(k, &h->props_gen, sizeof h->props_gen);  // (the section pairs' pointer, the kernel's form)
    k = fnv1a(k, &pt.tickets.ptr, sizeof pt.tickets.ptr);
  }
  if (tail >= 0) {
    // the step's whole GPU work but the assembly: setup, entry, the planned
    // batch of `tail` iterations (with the closing check, `tag` tells the two
    // forms apart, it may be 0), the finish, the post (mfea_step, batch_graph)
    k = fnv1a(k ^ 0xc0b0, &tail, sizeof tail);
    k = fnv1a(k, &tag, sizeof tag);
    k = fnv1a(k, &h->spec_strain, sizeof h->spec_strain);
    k = fnv1a(k, &h->mat, sizeof h->mat);  // (the post's stress kernel holds it by value)
    k = fnv1a(k, &h->props_gen, sizeof h->props_gen);  // (... and the property pointers, in its form for them)
    hipGraphExec_t& gc = h->graph_combo[form][tail];
    if (!gc || h->graph_combo_key[form][tail] != k) {
      if (gc) {
        HIPC(hipStreamSynchronize(s));
        (void)hipGraphExecDestroy(gc);
        gc = nullptr;
      }
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      if (head) enqueue_step_head(h, pt, head);
      if (start)
        launch_cg_init_finalize(s, pt.red.ptr, start->rtol, start->atol, start->norm, start->max_it, start->reg,
                                pt.state.ptr, pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
      if (!keep) enqueue_amg_setup(h, pt, reg);
      enqueue_amg_entry(h, pt, skip_init);
      enqueue_amg_chunk(h, pt, tail, close);
      launch_amg_finish(s, pt.amg.nd, pt.amg_cg, pt.x.ptr);
      const int prc = enqueue_post_work(h, h->spec_strain);
      const hipError_t ec = hipStreamEndCapture(s, &g);
      RC(prc);
      HIPC(ec);
      const hipError_t e = hipGraphInstantiate(&gc, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      h->graph_combo_key[form][tail] = k;
    }
    HIPC(hipGraphLaunch(gc, s));
    return 0;
  }
  hipGraphExec_t& gs = h->graph_setup[form];
  if (!gs || h->graph_setup_key[form] != k) {
    if (gs) {
      HIPC(hipStreamSynchronize(s));  // no replay of the old graph in flight
      (void)hipGraphExecDestroy(gs);
      gs = nullptr;
    }
    hipGraph_t g;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    if (head) enqueue_step_head(h, pt, head);
    if (start)
      launch_cg_init_finalize(s, pt.red.ptr, start->rtol, start->atol, start->norm, start->max_it, start->reg,
                              pt.state.ptr, pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
    if (!keep) enqueue_amg_setup(h, pt, reg);
    if (entry) enqueue_amg_entry(h, pt, skip_init);
    HIPC(hipStreamEndCapture(s, &g));
    const hipError_t e = hipGraphInstantiate(&gs, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPC(e);
    h->graph_setup_key[form] = k;
  }
  HIPC(hipGraphLaunch(gs, s));
  return 0;
}

int spec_post(mfea_handle* h);
int spec_undo(mfea_handle* h);
int assemble_impl(mfea_handle* h, mfea_stats* st, const double* rhs_dy);
int enqueue_post_work(mfea_handle* h, double max_strain);

int solve_amg(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o,
              mfea_stats* st) {
  Part& pt = part0(h);
  hipStream_t s = h->stream;
  bool rebuilt = false;
  HostLap clk;
  RC(ensure_amg(h, pt, &rebuilt, o->precond));
  clk.lap("ensure_amg");
  const int chunk = o->chunk > 0 ? solve_chunk_size(o) : 2;
  const SellOp op = sell_op(pt);
  const CgVecs v = cg_vecs(pt);
  const int nd = pt.amg.nd;
  // mfea_step's deferred assembly: at the head of the setup graph, or now
  const bool head = h->asm_pending && h->opt_graph && !h->opt_phase_times;
  if (h->asm_pending) {
    h->asm_pending = false;
    if (head) {
      HIPC(h->d_dy.alloc(2));
      k_written(h);  // (the head's k_assemble)
    } else {
      RC(assemble_impl(h, nullptr, h->h_red + 14));
    }
  }
  // the hierarchy's values are those this setup would form: skip it (the
  // iteration, entry and finish launches write vectors only — amg.hip)
  const uint64_t skey = amg_setup_key(h, pt, o->reg);
  const bool keep = h->opt_keep_operator && !pt.amg_cg.sweep && pt.kept.ok && pt.kept.key == skey &&
                    pt.kept.op_gen == h->op_gen && pt.kept.amg_gen == pt.amg_gen &&
                    pt.kept.fmask_gen == pt.fmask_gen;
  pt.kept.ok = false;  // (set again when this solve ends with status 0)
  pt.kept.key = skey;
  pt.kept.op_gen = h->op_gen;
  pt.kept.amg_gen = pt.amg_gen;
  pt.kept.fmask_gen = pt.fmask_gen;
  h->setup_skipped = keep;
  if (keep) ++h->amg_setup_kept;
  RC(phase_event(h, h->ev[1], s));
  // the CG start inside the setup graph when no phase event separates them
  const bool start_in_graph = h->opt_graph && h->opt_graph_start && !h->opt_phase_times && !head;
  // kept values (level 0's D⁻¹ and ω are current) and an RHS still to form:
  // the RHS, the CG's start and level-0 b as one launch (option amg_start)
  bool fused_start = false;
  if (!head) {
    // (mfea_step's assembly formed it for these displacements: AsmRhs)
    const bool rhs_done = h->rhs_fused && h->rhs_dy[0] == dy_top && h->rhs_dy[1] == dy_bot;
    h->rhs_fused = false;
    fused_start = h->opt_amg_start && keep && !rhs_done;
    if (fused_start) {
      if (pt.amg_inv_gen != pt.amg_gen || pt.amg_inv_row0 != pt.amg_cg.row0) {
        HIPC(pt.amg_inv.alloc(pt.P.n_nodes > 0 ? pt.P.n_nodes : 1));
        launch_amg_row0_inverse(s, pt.amg_cg, pt.amg_inv.ptr, pt.P.n_nodes);
        pt.amg_inv_gen = pt.amg_gen;
        pt.amg_inv_row0 = pt.amg_cg.row0;
      }
      launch_amg_start(s, nd, op, pt.code.ptr, dy_top, dy_bot, v, pt.partials.ptr, tix(pt, 0), pt.red.ptr,
                       pt.amg_lev[0], pt.amg_cg, pt.amg_inv.ptr, o->rtol, o->atol, o->norm, o->max_it, o->reg,
                       pt.state.ptr, pt.cg_part.ptr, 2 * 4 * kCgMaxPartials, h->bc.form(pt));
      ++h->amg_start_fused;
    } else {
      if (!rhs_done)
        launch_cg_rhs(s, op, pt.code.ptr, dy_top, dy_bot, o->reg, 2, v, pt.partials.ptr, tix(pt, 0), pt.red.ptr,
                      h->bc.form(pt));
      if (!start_in_graph)
        launch_cg_init_finalize(s, pt.red.ptr, o->rtol, o->atol, o->norm, o->max_it, o->reg, pt.state.ptr,
                                pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
    }
  }
  RC(phase_event(h, h->ev[2], s));
  // (phase times: the setup's end is an event between the setup and the entry)
  const bool entry = h->opt_graph && h->opt_setup_entry && !h->opt_phase_times;
  // the closing check (enqueue_amg_chunk): GAMG on the unpreconditioned norm
  // — PETSc's preconditioned norm needs M r for its test, and the sweep
  // preconditioners (SOR, ICC) keep the path they were measured on
  const bool close = h->opt_amg_close && o->norm == MFEA_NORM_UNPRECONDITIONED && pt.amg_kind == MFEA_PC_GAMG;
  // (every cached chunk graph is tagged: the two chunk forms never mix)
  // (−4,000,000: below the partitioned forms' ranges, −2,000,000 − x and −3,000,000 − x)
  // (lazy p, x: −8,000,000 more, so the four forms' ranges stay apart)
  const bool lazy = amg_lazy(h, pt);
  const int tag = -1000 - (int)(pt.amg_gen % 1000000) - (close ? 4000000 : 0) - (lazy ? 8000000 : 0);
  int64_t replays = 0;  // replay launches queued (read-only option amg_px_replays)
  // the converging update is iteration `iters`; update 0 ran in the entry, so
  // `iters` more groups (V-cycle, w, update) reach it: need.  With the closing
  // check the batch ends one group earlier, behind update iters − 1, and its
  // check finds what update `iters` would have (need may then be 0)
  const int planned = std::min(o->max_it, pt.amg_last_iters > 0 ? pt.amg_last_iters : 16);
  const int need = close ? std::max(0, planned - 1) : std::max(1, planned);
  int cycles = 1;  // preconditioner applications queued: the entry's, then one per group
  // mfea_step: the planned batch, the finish and the post as ONE graph of the
  // batch's exact length (option batch_graph), behind the setup in the same
  // graph (option combo_graph)
  const bool batch = h->spec_on && !h->ev_on && !h->spec_used && h->opt_batch_graph && !h->opt_phase_times &&
                     o->chunk <= 0 && need < mfea_handle::kRemGraphs && h->opt_graph;
  const bool combo = batch && entry && h->opt_combo_graph;
  // (combo: the graph reaches the batch's end and publishes the state; the
  // host's copy of the flag is cleared before it can)
  if (combo) h->h_state[0].done = 0;
  if (h->opt_graph) {
    // keep_operator on, a combined step that does set up (a new active set
    // in a run of kept steps): the setup as its own graph — one capture per
    // plan — in front of the combined graph WITHOUT it, which the kept steps
    // of this batch length replay anyway.  One combined graph with the setup
    // per length would be captured on exactly these steps (≈ 0.4 ms each,
    // more than the setup it holds); the extra graph launch costs a few µs.
    const bool split = combo && !keep && h->opt_keep_operator && !head;
    if (split) RC(launch_amg_setup_graph(h, pt, o->reg, skey, false));
    RC(launch_amg_setup_graph(h, pt, o->reg, skey, keep || split, entry, head ? o : nullptr,
                              start_in_graph && !fused_start ? o : nullptr, combo ? need : -1, tag, close,
                              fused_start));
  } else if (!keep) {
    enqueue_amg_setup(h, pt, o->reg);
  }
  clk.lap("to the setup graph");
  if (!entry) {
    RC(phase_event(h, h->ev_setup, s));
    h->ev_setup_used = true;
    enqueue_amg_entry(h, pt, fused_start);
  }
  HIPC(hipGetLastError());
  const bool no_graph = !h->opt_graph;
  SolveState fin;
  int rc;
  const auto drive_t0 = std::chrono::steady_clock::now();
  // x to row order behind every planned batch (see drive_planned)
  auto finish = [&]() -> int {
    launch_amg_finish(s, nd, pt.amg_cg, pt.x.ptr);
    HIPC(hipGetLastError());
    return spec_post(h);  // (mfea_step: the post behind the batch, one wait for both)
  };
  if (no_graph) {
    rc = drive_planned(h, chunk, o->max_it, need - 1,
                       [&]() -> int {
                         enqueue_amg_chunk(h, pt, chunk, close);
                         cycles += chunk;
                         if (lazy) replays += px_replays(chunk);
                         HIPC(hipGetLastError());
                         return 0;
                       },
                       &fin, finish);
  } else {
    auto capture = [&](hipGraphExec_t* ge, int n) -> int {
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      enqueue_amg_chunk(h, pt, n, close);
      HIPC(hipStreamEndCapture(s, &g));
      hipError_t e = hipGraphInstantiate(ge, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      return 0;
    };
    if (h->graph == nullptr || h->graph_chunk != chunk || h->graph_precond != MFEA_PC_GAMG ||
        h->graph_ell != tag) {
      destroy_graph(h);
      RC(capture(&h->graph, chunk));
      h->graph_chunk = chunk;
      h->graph_precond = MFEA_PC_GAMG;
      h->graph_ell = tag;
    }
    // the planned batch in long chunks (default solves only: a caller's
    // chunk size is kept as given); measured at C3 / C2: chunks of 8 in the
    // batch 2.24 / 1.15 ms per step against 2.36 / 1.20 with chunks of 2
    const int big = o->chunk > 0 ? chunk : h->opt_amg_big_chunk;
    if (big > chunk && (h->graph_big == nullptr || h->graph_big_chunk != big || h->graph_big_ell != tag)) {
      if (h->graph_big) (void)hipGraphExecDestroy(h->graph_big);
      h->graph_big = nullptr;
      RC(capture(&h->graph_big, big));
      h->graph_big_chunk = big;
      h->graph_big_ell = tag;
    }
    // the batch's remainder as ONE chunk of its own length (captured once per
    // length; the AMG iteration kernels keep no state across chunks that
    // depends on the chunk's parity): an odd iteration count no longer runs
    // one gated iteration — which costs as much as a live one — nor two
    // extra chunk boundaries (C3 at 15 iterations: 8 + 7 instead of 8 + 4×2)
    const int rem = big > chunk ? need - (need / big) * big : 0;
    const bool exact_rem = rem > 0 && rem != chunk && rem < mfea_handle::kRemGraphs;
    if (h->graph_rem_ell != tag) {  // another plan: the cached lengths hold its pointers
      for (auto& g : h->graph_rem) {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
      }
      h->graph_rem_ell = tag;
    }
    // (batch_graph: C2 / C3 two graph launches and four eager ones fewer per step)
    if (batch) {
      if (h->graph_batch_ell != tag || h->graph_batch_strain != h->spec_strain ||
          h->graph_batch_mat != h->mat_key()) {
        for (auto& g : h->graph_batch) {
          if (g) (void)hipGraphExecDestroy(g);
          g = nullptr;
        }
        h->graph_batch_ell = tag;
        h->graph_batch_strain = h->spec_strain;
        h->graph_batch_mat = h->mat_key();  // (the post's stress kernel holds them by value)
      }
      if (!combo && h->graph_batch[need] == nullptr) {
        hipGraph_t g;
        HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        enqueue_amg_chunk(h, pt, need, close);
        launch_amg_finish(s, nd, pt.amg_cg, pt.x.ptr);
        const int prc = enqueue_post_work(h, h->spec_strain);
        const hipError_t ec = hipStreamEndCapture(s, &g);
        RC(prc);
        HIPC(ec);
        hipError_t e = hipGraphInstantiate(&h->graph_batch[need], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIPC(e);
      }
      rc = drive_batch(h, chunk, o->max_it, need,
                       [&]() -> int {
                         if (!combo) HIPC(hipGraphLaunch(h->graph_batch[need], s));  // (combo: launched with the setup)
                         cycles += need;
                         if (lazy) replays += px_replays(need);
                         return 0;
                       },
                       [&](int n) -> int {
                         HIPC(hipGraphLaunch(h->graph, s));
                         cycles += n;
                         if (lazy) replays += px_replays(chunk);
                         return 0;
                       },
                       &fin, finish, combo);
    } else {
      // (need 0: the closing check alone, a chunk of length 0 among the remainders)
      const int odd = need == 0 ? 0 : rem;
      if ((exact_rem || need == 0) && h->graph_rem[odd] == nullptr) RC(capture(&h->graph_rem[odd], odd));
      rc = drive_sized(h, big, chunk, o->max_it, need - 1,
                       [&](int n) -> int {
                         HIPC(hipGraphLaunch(n == chunk ? h->graph : n == big ? h->graph_big : h->graph_rem[n], s));
                         cycles += n;
                         if (lazy) replays += px_replays(n);
                         return 0;
                       },
                       &fin, finish, exact_rem, close);
    }
  }
  h->amg_px_replays += replays;
  if (rc) return rc;
  h->amg_last_cycles = cycles;
  if (fin.status == 0 && fin.closed) ++h->amg_close_hits;
  if (fin.status != 0) RC(spec_undo(h));
  clk.lap("solve (setup + iterations)", fin.iters);
  if (fin.status != 0 && pt.amg_reused) {
    // a hierarchy kept from another active set failed: rebuild for this one
    // before anything else is blamed (the ω retry below would otherwise run
    // on the kept hierarchy)
    pt.amg_stale = true;
    RC(sync_stream(h));
    return solve_amg(h, dy_top, dy_bot, o, st);
  }
  if (pt.amg_lev.size() > 1 && pt.amg_kind == MFEA_PC_GAMG &&
      omega_suspect(h, fin.status, o->max_it, std::max(pt.amg_build_iters, pt.amg_last_iters)))
    return omega_retry(h, [&]() { return solve_amg(h, dy_top, dy_bot, o, st); });
  if (fin.status == 0) pt.amg_last_iters = fin.iters;
  if (fin.status == 0 && !pt.amg_reused) {
    pt.amg_build_iters = fin.iters;  // the hierarchy on the set it was built for
  } else if (pt.amg_reused && pt.amg_build_iters >= 0) {
    // rent or buy: the iterations above the hierarchy's own count cost this
    // solve's time per iteration; once that rent adds up to the last build's
    // time, or one solve needs far more (amg_rebuild_pct), rebuild
    const double t_it = std::chrono::duration<double>(std::chrono::steady_clock::now() - drive_t0).count() /
                        std::max<int64_t>(1, fin.closed ? fin.iters : fin.iters + 1);  // (the cycles it took)
    if (fin.iters > pt.amg_build_iters) pt.amg_excess_s += (fin.iters - pt.amg_build_iters) * t_it;
    const bool rent_due = h->opt_amg_rebuild_rent > 0 &&
                          pt.amg_excess_s >= pt.amg_build_s * h->opt_amg_rebuild_rent / 100.0;
    if (rent_due || fin.iters > (int64_t)pt.amg_build_iters * h->opt_amg_rebuild_pct / 100 + 2)
      pt.amg_stale = true;  // degraded: the next solve rebuilds for its active set
  }
  rc = finish_solve(h, fin, st);
  // (no retry or rebuild above re-formed them since: those paths returned)
  if (rc == 0 && fin.status == 0) pt.kept.ok = true;
  if (st) {
    st->amg_levels = (int32_t)pt.amg_lev.size();
    st->amg_rebuilt = rebuilt ? 1 : 0;
  }
  return rc;
}

// ---------------------------------------------------------------------------
// Distributed GAMG over ONE global hierarchy (option "amg_dist" 1, the
// default of partitioned handles).  Every rank builds the same
// hierarchy from the whole mesh — the one-partition hierarchy, so the solve
// needs the one-partition iteration count — and computes only its own rows of
// the split levels (amg.hpp AmgRank); the values a rank's rows read from
// other ranks arrive through the exchanges below.  Levels of at most
// "amg_rep_rows" rows are replicated: every rank holds and computes all of them.
// ---------------------------------------------------------------------------
// The global element activity (original order).  Partitions on one device:
// each partition's own elements; RCCL: a max-all-reduce of E bytes (a rank
// contributes the elements it reports, 0 elsewhere).
int global_active(mfea_handle* h, std::vector<uint8_t>& key) {
  if (h->gkey_gen == h->act_gen && (int64_t)h->gkey.size() == h->Ecount) {
    key = h->gkey;  // kept current by mfea_set_active and the failed-id exchange
    return 0;
  }
  key.assign(h->Ecount, 0);
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int64_t E = pt.P.n_elems;
    std::vector<uint8_t> a(E);
    if (E) HIPC(hmemcpy(h, a.data(), pt.active.ptr, E, hipMemcpyDeviceToHost));
    for (int64_t le = 0; le < E; ++le)
      if (pt.plan.elem_own[le]) key[pt.plan.elem_g[le]] = a[le];
  }
  if (h->world > 1 && h->Ecount) {
    HIPC(h->gact.alloc(h->Ecount));
    HIPC(hipMemcpyAsync(h->gact.ptr, key.data(), h->Ecount, hipMemcpyHostToDevice, h->stream));
    NCCLC(ncclAllReduce(h->gact.ptr, h->gact.ptr, (size_t)h->Ecount, ncclUint8, ncclMax, h->comm, h->stream));
    HIPC(hipMemcpyAsync(key.data(), h->gact.ptr, h->Ecount, hipMemcpyDeviceToHost, h->stream));
    RC(sync_stream(h));
  }
  h->gkey = key;
  h->gkey_gen = h->act_gen;
  return 0;
}

// the partition's exchange plans on the device (item lists carved from one
// allocation) and staging buffers for the largest transfer
int upload_xplans(mfea_handle* h, Part& pt) {
  const AmgRank& rk = pt.amg_rank;
  const int nd = h->gamg.nd;
  size_t stage = 1;
  IndexStage st(1, /*gap=*/1);  // (the gap: empty lists get offsets of their own)
  int pass = 0;
  auto put = [&](const XPlan& x, int width_bytes) -> Part::XDev {
    stage = std::max(stage, (size_t)std::max(x.n_send(), x.n_recv()) * width_bytes);
    const size_t s = st.put(x.sidx), r = st.put(x.ridx);
    Part::XDev d;
    d.x = &x;
    d.s = pass == 0 ? nullptr : pt.amg_xi.ptr + s;
    d.r = pass == 0 ? nullptr : pt.amg_xi.ptr + r;
    return d;
  };
  for (pass = 0; pass < 2; ++pass) {  // count, then fill
    if (pass == 1) {
      RC(stage_begin(pt.amg_xi, st));
      HIPC(pt.amg_xs.alloc(stage / 8 + 1));
      HIPC(pt.amg_xr.alloc(stage / 8 + 1));
    }
    pt.xd_a.clear();
    pt.xd_r.clear();
    pt.xd_p.clear();
    pt.xd_sp.clear();
    pt.xd_sap.clear();
    for (const auto& x : rk.xa) pt.xd_a.push_back(put(x, 4 * nd));
    for (const auto& x : rk.xr) pt.xd_r.push_back(put(x, 4 * nd));
    for (const auto& x : rk.xp) pt.xd_p.push_back(put(x, 4 * nd));
    pt.xd_g = put(rk.xg, 4 * nd);
    for (const auto& x : rk.sp) pt.xd_sp.push_back(put(x, 8 * nd * nd));
    for (const auto& x : rk.sap) pt.xd_sap.push_back(put(x, 8 * nd * nd));
    pt.xd_sg = put(rk.sg, 8 * nd * nd);
    pt.xd_c = put(rk.xc, 4 * nd);
    pt.xd_spt = put(rk.spt, 4 * nd * nd);
    pt.xd_sd = put(rk.sd, 4 * nd * nd);
  }
  return stage_flush(h, pt.amg_xi, st);
}

// the distributed V-cycle in its compact form (option amg_dist_cycle)
bool dist_compact(const mfea_handle* h) { return h->opt_amg_dist_cycle == 1 && h->opt_amg_cycle == 1; }

// (Re)build the global hierarchy (host) when the element activity may have
// changed (act_gen) and actually did.
int ensure_gamg_plan(mfea_handle* h, bool* rebuilt) {
  *rebuilt = false;
  bool host_ok = h->gamg_ok && h->gamg_act_gen == h->act_gen;
  if (!host_ok && h->gamg_ok) {
    std::vector<uint8_t> key;
    RC(global_active(h, key));
    host_ok = key == h->gamg_key;
    if (host_ok) h->gamg_act_gen = h->act_gen;
  }
  if (!host_ok) {
    std::vector<uint8_t> key;
    RC(global_active(h, key));
    h->gamg_ok = false;
    AmgDistSpec spec;
    spec.world = nranks(h);
    const bool compact = dist_compact(h);
    spec.rep_rows = compact ? INT64_MAX : h->opt_amg_rep_rows;
    spec.owner.resize(h->gpat.n_free);
    for (int64_t i = 0; i < h->gpat.n_free; ++i) spec.owner[i] = h->gowner[h->gpat.perm[i]];
    std::string err = build_amg(h->gpat, key, lane_dofs(h), h->gamg, h->opt_amg_max_levels, &spec,
                                amg_strength(h));
    if (!err.empty()) return fail(MFEA_EINVAL, "AMG setup: " + err);
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      err = build_amg_rank(h->gamg, pt.rank, pt.amg_rank);
      if (!compact) pt.amg_rank.compact = false;  // (a four-step plan split at level 0 only)
      if (err.empty())
        err = build_amg_level0(h->gamg, h->gpat, pt.amg_rank, pt.P, pt.plan.node_g, pt.plan.elem_g, key, pt.g_a0,
                               pt.g_row0);
      if (!err.empty()) return fail(MFEA_EINVAL, "AMG setup: " + err);
      pt.dev_plan = -1;
    }
    h->gamg_key = std::move(key);
    h->gamg_ok = true;
    h->gamg_act_gen = h->act_gen;
    ++h->gamg_plan_gen;
    *rebuilt = true;
  }
  return 0;
}

// ... and have the device arrays hold it (they may hold the block-Jacobi plans)
int ensure_gamg(mfea_handle* h, bool* rebuilt) {
  RC(ensure_gamg_plan(h, rebuilt));
  bool up = false;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    if (pt.dev_plan == 1) continue;
    if (!up) RC(drain_before_upload(h, "plan upload"));
    if (!up) destroy_graph(h);
    up = true;
    RC(upload_amg(h, pt, h->gamg, &pt.amg_rank, &pt.g_a0, &pt.g_row0));
    RC(upload_xplans(h, pt));
    AmgDist& d = pt.amg_dist;
    d = AmgDist{};
    d.rank = pt.rank;
    d.gall[0] = pt.dv.gall[0];
    d.gall[1] = pt.dv.gall[1];
    d.gsend = pt.dv.gsend;
    d.zero_w = h->world > 1 && h->opt_dist_sums == 1 ? h->world : 0;
    pt.dev_plan = 1;
  }
  if (up) ++h->gamg_gen;
  return 0;
}

// One exchange of the distributed GAMG on every partition: pack the items of
// plan(pt) from vec(pt) (width scalars of `bytes` each), one RCCL group of
// point-to-point transfers (partitions on one device: device copies), unpack
// into the same array.
template <class GetPlan, class GetVec>
int gx(mfea_handle* h, GetPlan plan, GetVec vec, int width, int bytes) {
  hipStream_t s = h->stream;
  if (h->world <= 1) {  // partitions on one device: every transfer in one launch, array to array
    XPairs pr;
    for (auto& a : h->parts) {
      const Part::XDev& da = plan(*a);
      const XPlan& xa = *da.x;
      for (size_t i = 0; i < xa.peers.size(); ++i) {
        if (!xa.scnt[i]) continue;
        Part& b = *h->parts[xa.peers[i]];
        const Part::XDev& db = plan(b);
        const XPlan& xb = *db.x;
        const auto it = std::lower_bound(xb.peers.begin(), xb.peers.end(), a->rank);
        const size_t jb = (size_t)(it - xb.peers.begin());
        if (it == xb.peers.end() || *it != a->rank || xb.rcnt[jb] != xa.scnt[i])
          return fail(MFEA_EINVAL, "internal: asymmetric GAMG exchange plan");
        if (pr.n == kMaxXPairs) {
          launch_xcopy(s, pr, width, bytes);
          pr = XPairs();
        }
        pr.src[pr.n] = vec(*a);
        pr.dst[pr.n] = vec(b);
        pr.sidx[pr.n] = da.s + xa.soff[i];
        pr.ridx[pr.n] = db.r + xb.roff[jb];
        pr.off[pr.n + 1] = pr.off[pr.n] + xa.scnt[i];
        ++pr.n;
      }
    }
    launch_xcopy(s, pr, width, bytes);
    HIPC(hipGetLastError());
    return 0;
  }
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Part::XDev& d = plan(pt);
    launch_xpack(s, vec(pt), d.s, d.x->n_send(), width, bytes, pt.amg_xs.ptr);
  }
  HIPC(hipGetLastError());
  const size_t item = (size_t)width * bytes;
  if (h->world > 1) {
    Part& pt = part0(h);
    const XPlan& x = *plan(pt).x;
    if (!x.peers.empty()) {
      const ncclDataType_t t = bytes == 8 ? ncclFloat64 : ncclFloat32;
      char* sb = reinterpret_cast<char*>(pt.amg_xs.ptr);
      char* rb = reinterpret_cast<char*>(pt.amg_xr.ptr);
      NCCLC(ncclGroupStart());
      for (size_t i = 0; i < x.peers.size(); ++i) {
        if (x.scnt[i])
          NCCLC(ncclSend(sb + x.soff[i] * item, (size_t)(x.scnt[i] * width), t, x.peers[i], h->comm, s));
        if (x.rcnt[i])
          NCCLC(ncclRecv(rb + x.roff[i] * item, (size_t)(x.rcnt[i] * width), t, x.peers[i], h->comm, s));
      }
      NCCLC(ncclGroupEnd());
    }
  } else {
    for (auto& a : h->parts) {
      const XPlan& xa = *plan(*a).x;
      for (size_t i = 0; i < xa.peers.size(); ++i) {
        if (!xa.scnt[i]) continue;
        Part& b = *h->parts[xa.peers[i]];
        const XPlan& xb = *plan(b).x;
        const auto it = std::lower_bound(xb.peers.begin(), xb.peers.end(), a->rank);
        const size_t jb = (size_t)(it - xb.peers.begin());
        if (it == xb.peers.end() || *it != a->rank || xb.rcnt[jb] != xa.scnt[i])
          return fail(MFEA_EINVAL, "internal: asymmetric GAMG exchange plan");
        HIPC(hipMemcpyAsync(reinterpret_cast<char*>(b.amg_xr.ptr) + xb.roff[jb] * item,
                            reinterpret_cast<const char*>(a->amg_xs.ptr) + xa.soff[i] * item, xa.scnt[i] * item,
                            hipMemcpyDeviceToDevice, s));
      }
    }
  }
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Part::XDev& d = plan(pt);
    launch_xunpack(s, pt.amg_xr.ptr, d.r, d.x->n_recv(), width, bytes, vec(pt));
  }
  HIPC(hipGetLastError());
  return 0;
}

// level l's Gershgorin bound: the maximum over the ranks (every rank then
// takes the same smoother weight ω_l and forms the same P_l)
int bound_max(mfea_handle* h, int l) {
  if (h->world > 1) {
    double* om = part0(h).amg_lev[l].omega + 1;
    NCCLC(ncclAllReduce(om, om, 1, ncclFloat64, ncclMax, h->comm, h->stream));
    return 0;
  }
  std::vector<double*> oms;
  for (auto& pp : h->parts) oms.push_back(pp->amg_lev[l].omega);
  launch_amg_bound_max(h->stream, oms.data(), (int)oms.size());
  HIPC(hipGetLastError());
  return 0;
}

// the per-solve numeric setup, split levels with their exchanges
int enqueue_gamg_setup(mfea_handle* h, double reg) {
  hipStream_t s = h->stream;
  const AmgPlan& pl = h->gamg;
  const int nd = pl.nd, nb2 = nd * nd, nlev = (int)pl.lev.size(), ns = pl.n_dist;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_a0(s, nd, pt.amg_lev[0], sell_op(pt), pt.amg_cg.row0, pt.amg_a0_ptr, pt.amg_a0_a, reg);
  }
  HIPC(hipGetLastError());
  RC(bound_max(h, 0));
  for (int l = 0; l < nlev; ++l) {
    const bool split = l < ns;
    auto stage = [&](int st) -> int {
      for (auto& pp : h->parts) {
        Part& pt = *pp;
        launch_amg_level_setup(s, nd, pt.amg_lev[l], l + 1 < nlev ? &pt.amg_lev[l + 1] : nullptr, l == 0, st);
      }
      HIPC(hipGetLastError());
      return 0;
    };
    if (l > 0) {
      RC(stage(kSetupDinv));
      if (split) RC(bound_max(h, l));
    }
    if (pl.lev[l].coarsest) break;
    RC(stage(kSetupP));
    if (split)
      RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_sp[l]; },
            [l](Part& p) -> void* { return p.amg_lev[l].P.val32; }, nb2, 4));
    RC(stage(kSetupAP));
    if (split)
      RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_sap[l]; },
            [l](Part& p) -> void* { return p.amg_lev[l].apval; }, nb2, 4));
    RC(stage(kSetupAC));
    if (l + 1 == ns && ns < nlev) {  // level ns is replicated: gather its A
      RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_sg; },
            [ns](Part& p) -> void* { return p.amg_lev[ns].A.val32; }, nb2, 4));
    }
  }
  if (part0(h).amg_rank.compact && nlev > 1) {
    // the compact operators: level 0's Ã_0 and P̃_0 on this rank's rows; the
    // P̃_0 blocks and level-0 diagonal blocks other ranks' R̂_0 rows read; its
    // own R̂_0 rows; the replicated levels whole, then their collapse
    for (auto& pp : h->parts)
      launch_amg_compact_level(s, nd, pp->amg_lev.data(), 0, kCompactPT | kCompactAT);
    HIPC(hipGetLastError());
    RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_spt; },
          [](Part& p) -> void* { return p.amg_lev[0].PT.val32; }, nb2, 4));
    RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_sd; },
          [](Part& p) -> void* { return p.amg_lev[0].A.val32; }, nb2, 4));
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_amg_compact_level(s, nd, pt.amg_lev.data(), 0, kCompactRT);
      launch_amg_compact_setup(s, nd, pt.amg_lev.data(), nlev, pt.amg_cg.coll, 1);
    }
    HIPC(hipGetLastError());
  }
  return 0;
}

// One distributed V-cycle on every partition (gate: iteration j's flag;
// j < 0: ungated, the solve's first cycle)
int enqueue_gamg_vcycle(mfea_handle* h, int j) {
  hipStream_t s = h->stream;
  const AmgPlan& pl = h->gamg;
  const int nd = pl.nd, nlev = (int)pl.lev.size(), ns = pl.n_dist;
  if (nlev <= 1) return 0;  // the update's vcycle_entry solved the only level
  if (part0(h).amg_rank.compact) {
    // split at level 0 only: x_0 halo → down_0 (this rank's R̂_0 rows into
    // x_1, its Ã_0 rows into c_0) → x_1 all-gather → the replicated compact
    // cycle from level 1 (collapsed as on one partition) → up_0 on this
    // rank's P̃_0 rows into u.  Three exchange points with the u halo.
    RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_c; }, [](Part& p) -> void* { return p.amg_lev[0].x; },
          nd, 4));
    for (auto& pp : h->parts) launch_amg_down(s, nd, pp->amg_lev[0], pp->amg_lev[1]);
    HIPC(hipGetLastError());
    RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_g; }, [](Part& p) -> void* { return p.amg_lev[1].x; },
          nd, 4));
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_amg_vcycle(s, nd, pt.amg_lev.data(), nlev, pt.amg_cg, 0, nullptr, 1);
      launch_amg_up(s, nd, pt.amg_lev[0], pt.amg_lev[1], pt.amg_cg.u);
    }
    HIPC(hipGetLastError());
    return 0;
  }
  const int top = std::min(ns, nlev - 1);  // split levels with a level below
  (void)j;  // no gate (enqueue_amg_chunk): past the stop every launch rewrites the same values
  auto gate = [](Part&) -> const int32_t* { return nullptr; };
  auto steps = [&](int l, int step) {
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_amg_vstep(s, nd, pt.amg_lev.data(), l, pt.amg_cg, step, gate(pt));
    }
  };
  for (int l = 0; l < top; ++l) {
    RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_a[l]; },
          [l](Part& p) -> void* { return p.amg_lev[l].x; }, nd, 4));
    steps(l, kStepResid);
    HIPC(hipGetLastError());
    RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_r[l]; },
          [l](Part& p) -> void* { return p.amg_lev[l].t; }, nd, 4));
    steps(l, kStepRestrict);
    HIPC(hipGetLastError());
  }
  if (ns < nlev) {  // the replicated levels: gather level ns's b, every rank runs them whole
    RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_g; },
          [ns](Part& p) -> void* { return p.amg_lev[ns].b; }, nd, 4));
    for (auto& pp : h->parts) {
      Part& pt = *pp;
      launch_amg_xinit_rows(s, nd, pt.amg_lev[ns], pt.xd_g.r, pt.xd_g.x->n_recv(), gate(pt));
      launch_amg_vcycle(s, nd, pt.amg_lev.data(), nlev, pt.amg_cg, pt.amg_tail, gate(pt), ns);
    }
    HIPC(hipGetLastError());
  }
  for (int l = top - 1; l >= 0; --l) {
    if (l + 1 < ns) {  // the coarse output of a split level
      const bool co = pl.lev[l + 1].coarsest;
      RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_p[l]; },
            [l, co](Part& p) -> void* { return co ? p.amg_lev[l + 1].x : p.amg_lev[l + 1].e; }, nd, 4));
    }
    steps(l, kStepProlong);
    HIPC(hipGetLastError());
    RC(gx(h, [l](Part& p) -> const Part::XDev& { return p.xd_a[l]; },
          [l](Part& p) -> void* { return p.amg_lev[l].x; }, nd, 4));
    steps(l, kStepPost);
    HIPC(hipGetLastError());
  }
  return 0;
}

// one distributed GAMG iteration j: update (gathered sums) → V-cycle → u halo
// → w = A_0 u → this rank's sums → all-gather of the sums
int enqueue_gamg_iteration(mfea_handle* h, int j) {
  hipStream_t s = h->stream;
  const int nd = h->gamg.nd;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_update(s, nd, j, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.state.ptr, pt.cg_part.ptr,
                         &pt.amg_dist);
  }
  HIPC(hipGetLastError());
  RC(enqueue_gamg_vcycle(h, j));
  RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_a[0]; }, [](Part& p) -> void* { return p.amg_cg.u; },
        nd, 4));
  const int q = (j & 1) ^ 1;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_w(s, nd, j, false, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr);
    launch_amg_gsum(s, pt.amg_cg, cg_part_buf(pt, q), pt.amg_dist, q);
  }
  HIPC(hipGetLastError());
  return xchg_sums(h, q);
}

int enqueue_gamg_chunk(mfea_handle* h, int chunk) {
  for (int j = 0; j < chunk; ++j) RC(enqueue_gamg_iteration(h, j));
  for (auto& pp : h->parts) launch_cg_advance(h->stream, chunk, pp->slots.ptr, pp->state.ptr, pp->mirror);
  HIPC(hipGetLastError());
  return 0;
}

int solve_gamg_global(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o, mfea_stats* st) {
  hipStream_t s = h->stream;
  bool rebuilt = false;
  RC(ensure_gamg(h, &rebuilt));
  const int chunk = o->chunk > 0 ? solve_chunk_size(o) : 2;
  const int W = nranks(h);
  const int nd = h->gamg.nd;
  RC(phase_event(h, h->ev[1], s));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_cg_rhs(s, sell_op(pt), pt.code.ptr, dy_top, dy_bot, o->reg, 2, cg_vecs(pt), pt.partials.ptr, tix(pt, 0),
                  pt.red.ptr);
  }
  RC(gather4(h, 0));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rank_sum(s, pt.gred, W, pt.red.ptr + 12);
    launch_cg_init_finalize(s, pt.red.ptr + 12, o->rtol, o->atol, o->norm, o->max_it, o->reg, pt.state.ptr,
                            pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
  }
  RC(phase_event(h, h->ev[2], s));
  RC(enqueue_gamg_setup(h, o->reg));
  RC(phase_event(h, h->ev_setup, s));
  h->ev_setup_used = true;
  // iteration 0's u and w: the V-cycle of r₀, ungated
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_init(s, nd, pt.amg_lev[0], pt.amg_cg, cg_vecs(pt).r[0]);
  }
  RC(enqueue_gamg_vcycle(h, -1));
  RC(gx(h, [](Part& p) -> const Part::XDev& { return p.xd_a[0]; }, [](Part& p) -> void* { return p.amg_cg.u; },
        nd, 4));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_w(s, nd, 0, true, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr);
    launch_amg_gsum(s, pt.amg_cg, cg_part_buf(pt, 0), pt.amg_dist, 0);
  }
  RC(xchg_sums(h, 0));
  HIPC(hipGetLastError());
  const int tag = -3000000 - (int)(h->gamg_gen % 1000000);
  Part& p0 = part0(h);
  const int expected = std::min(o->max_it, p0.amg_last_iters > 0 ? p0.amg_last_iters : 16);
  SolveState fin;
  if (!h->opt_dist_graph) {
    RC(drive_planned(h, chunk, o->max_it, expected, [&]() -> int { return enqueue_gamg_chunk(h, chunk); }, &fin));
  } else {
    if (h->graph == nullptr || h->graph_chunk != chunk || h->graph_precond != MFEA_PC_GAMG || h->graph_ell != tag) {
      destroy_graph(h);
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      const int rc = enqueue_gamg_chunk(h, chunk);
      const hipError_t ce = hipStreamEndCapture(s, &g);
      if (rc) return rc;
      HIPC(ce);
      hipError_t e = hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      h->graph_chunk = chunk;
      h->graph_precond = MFEA_PC_GAMG;
      h->graph_ell = tag;
    }
    RC(drive_planned(h, chunk, o->max_it, expected,
                     [&]() -> int {
                       HIPC(hipGraphLaunch(h->graph, s));
                       return 0;
                     },
                     &fin));
  }
  if (omega_suspect(h, fin.status, o->max_it, p0.amg_last_iters))
    return omega_retry(h, [&]() { return solve_gamg_global(h, dy_top, dy_bot, o, st); });
  if (fin.status == 0) p0.amg_last_iters = fin.iters;
  // x to row order, then the displacement halo (ghost rows of the post kernels)
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_finish(s, nd, pt.amg_cg, pt.x.ptr);
    launch_rows_pack(s, pt.xsend_rows.ptr, (int64_t)pt.plan.xsend_node.size(), pt.x.ptr, pt.xh_send);
  }
  RC(xchg_xhalo(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rows_unpack(s, pt.xrecv_rows.ptr, (int64_t)pt.plan.xrecv_node.size(), pt.xh_recv, pt.x.ptr);
  }
  HIPC(hipGetLastError());
  const int rc = finish_solve(h, fin, st);
  if (st) {
    st->amg_levels = (int32_t)h->gamg.lev.size();
    st->amg_rebuilt = rebuilt ? 1 : 0;
  }
  return rc;
}

// The partitioned GAMG solve: block-Jacobi-over-partitions AMG V-cycles inside
// a global CG (amg.hpp AmgHalo), the exchanges of enqueue_amg_dist_iteration.
int solve_amg_dist(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o,
                   mfea_stats* st) {
  hipStream_t s = h->stream;
  bool rebuilt = false;
  for (auto& pp : h->parts) {
    bool rb = false;
    RC(ensure_amg(h, *pp, &rb));
    rebuilt = rebuilt || rb;
  }
  const int chunk = o->chunk > 0 ? solve_chunk_size(o) : 2;
  const int W = nranks(h);
  RC(phase_event(h, h->ev[1], s));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_cg_rhs(s, sell_op(pt), pt.code.ptr, dy_top, dy_bot, o->reg, 2, cg_vecs(pt), pt.partials.ptr,
                  tix(pt, 0), pt.red.ptr);
  }
  RC(gather4(h, 0));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rank_sum(s, pt.gred, W, pt.red.ptr + 12);
    launch_cg_init_finalize(s, pt.red.ptr + 12, o->rtol, o->atol, o->norm, o->max_it, o->reg, pt.state.ptr,
                            pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
  }
  RC(phase_event(h, h->ev[2], s));
  for (auto& pp : h->parts) enqueue_amg_setup(h, *pp, o->reg);
  RC(phase_event(h, h->ev_setup, s));
  h->ev_setup_used = true;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int nd = pt.amg.nd;
    launch_amg_cg_init(s, nd, pt.amg_lev[0], pt.amg_cg, cg_vecs(pt).r[0]);
    launch_amg_vcycle(s, nd, pt.amg_lev.data(), (int)pt.amg_lev.size(), pt.amg_cg,
                      pt.amg_tail, nullptr);
    launch_amg_pack_u(s, nd, pt.amg_cg, pt.amg_dist);
  }
  RC(xchg_u(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_cg_w(s, pt.amg.nd, 0, true, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr,
                    &pt.amg_dist);
    launch_amg_gsum(s, pt.amg_cg, cg_part_buf(pt, 0), pt.amg_dist, 0);
  }
  RC(xchg_sums(h, 0));
  HIPC(hipGetLastError());
  int64_t gen = 0;
  for (auto& pp : h->parts) gen = gen * 1000003 + pp->amg_gen;
  const int tag = -2000000 - (int)(gen % 1000000);
  Part& p0 = part0(h);
  const int expected = std::min(o->max_it, p0.amg_last_iters > 0 ? p0.amg_last_iters : 16);
  SolveState fin;
  if (!h->opt_dist_graph) {
    RC(drive_planned(h, chunk, o->max_it, expected, [&]() -> int { return enqueue_amg_dist_chunk(h, chunk); },
                     &fin));
  } else {
    if (h->graph == nullptr || h->graph_chunk != chunk || h->graph_precond != MFEA_PC_GAMG ||
        h->graph_ell != tag) {
      destroy_graph(h);
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      const int rc = enqueue_amg_dist_chunk(h, chunk);
      const hipError_t ce = hipStreamEndCapture(s, &g);
      if (rc) return rc;
      HIPC(ce);
      hipError_t e = hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      h->graph_chunk = chunk;
      h->graph_precond = MFEA_PC_GAMG;
      h->graph_ell = tag;
    }
    RC(drive_planned(h, chunk, o->max_it, expected,
                     [&]() -> int {
                       HIPC(hipGraphLaunch(h->graph, s));
                       return 0;
                     },
                     &fin));
  }
  if (omega_suspect(h, fin.status, o->max_it, p0.amg_last_iters))
    return omega_retry(h, [&]() { return solve_amg_dist(h, dy_top, dy_bot, o, st); });
  if (fin.status == 0) p0.amg_last_iters = fin.iters;
  // x to row order, then the displacement halo (ghost rows of the post kernels)
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_amg_finish(s, pt.amg.nd, pt.amg_cg, pt.x.ptr);
    launch_rows_pack(s, pt.xsend_rows.ptr, (int64_t)pt.plan.xsend_node.size(), pt.x.ptr, pt.xh_send);
  }
  RC(xchg_xhalo(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rows_unpack(s, pt.xrecv_rows.ptr, (int64_t)pt.plan.xrecv_node.size(), pt.xh_recv, pt.x.ptr);
  }
  HIPC(hipGetLastError());
  const int rc = finish_solve(h, fin, st);
  if (st) {
    st->amg_levels = (int32_t)p0.amg_lev.size();
    st->amg_rebuilt = rebuilt ? 1 : 0;
  }
  return rc;
}

// The partitioned solve: the same CG-CG iterations on every partition's lanes,
// with the exchanges of partition.hpp between kernels.
int solve_dist(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o,
               mfea_stats* st) {
  hipStream_t s = h->stream;
  const int precond = o->precond == MFEA_PC_BLOCK_JACOBI ? 1 : 0;
  const int chunk = solve_chunk_size(o);
  const int W = nranks(h);
  RC(phase_event(h, h->ev[1], s));
  // RHS, M⁻¹ and the global (‖b‖², ‖M⁻¹b‖²)
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_cg_rhs(s, sell_op(pt), pt.code.ptr, dy_top, dy_bot, o->reg, precond, cg_vecs(pt),
                  pt.partials.ptr, tix(pt, 0), pt.red.ptr);
  }
  RC(gather4(h, 0));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rank_sum(s, pt.gred, W, pt.red.ptr + 12);
    launch_cg_init_finalize(s, pt.red.ptr + 12, o->rtol, o->atol, o->norm, o->max_it, o->reg,
                            pt.state.ptr,
                            pt.cg_part.ptr, 2 * 4 * kCgMaxPartials);
    launch_ell_init(s, ell_op(h, pt), sell_op(pt), precond, cg_vecs(pt), ell_vecs(pt));
    launch_ell_pack0(s, ell_op(h, pt), precond, ell_vecs(pt), pt.dv);
  }
  RC(xchg_records(h, 1, false));  // [r₀ | M] of the cut rows
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_ell_first(s, ell_op(h, pt), o->reg, precond, ell_vecs(pt), pt.slots.ptr, pt.cg_part.ptr,
                     &pt.dv);
    launch_psum(s, ell_op(h, pt), cg_part_buf(pt, 0), pt.dv.gall[0] + 4 * pt.rank, pt.dv.gsend);
  }
  RC(xchg_records(h, 0, true));
  HIPC(hipGetLastError());
  RC(phase_event(h, h->ev[2], s));
  // each chunk (kernels + exchanges) replays as one hipGraph (option
  // "dist_graph" 0: eager launches)
  const bool dist_graph = h->opt_dist_graph;
  SolveState fin;
  if (dist_graph) {
    const int tag = -10 - lane_dofs(h);  // graph_ell key of the partitioned chunk
    if (h->graph == nullptr || h->graph_chunk != chunk || h->graph_precond != precond ||
        h->graph_ell != tag) {
      destroy_graph(h);
      hipGraph_t g;
      HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      const int rc = enqueue_chunk_dist(h, chunk, precond);
      const hipError_t ce = hipStreamEndCapture(s, &g);
      if (rc) return rc;
      HIPC(ce);
      hipError_t e = hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      HIPC(e);
      h->graph_chunk = chunk;
      h->graph_precond = precond;
      h->graph_ell = tag;
    }
    RC(drive_chunks(
        h, chunk, o->max_it,
        [&]() -> int {
          HIPC(hipGraphLaunch(h->graph, s));
          return 0;
        },
        &fin, /*mirror=*/true));
  } else {
    RC(drive_chunks(
        h, chunk, o->max_it, [&]() -> int { return enqueue_chunk_dist(h, chunk, precond); }, &fin,
        /*mirror=*/true));
  }
  // x to row order, then the displacement halo (ghost rows of the post kernels)
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_ell_finish(s, ell_op(h, pt), ell_vecs(pt), pt.x.ptr);
    launch_rows_pack(s, pt.xsend_rows.ptr, (int64_t)pt.plan.xsend_node.size(), pt.x.ptr, pt.xh_send);
  }
  RC(xchg_xhalo(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    launch_rows_unpack(s, pt.xrecv_rows.ptr, (int64_t)pt.plan.xrecv_node.size(), pt.xh_recv,
                       pt.x.ptr);
  }
  HIPC(hipGetLastError());
  return finish_solve(h, fin, st);
}

// the element colouring of pt's pattern on the device (symbolic.hpp
// build_elem_colour), once per pattern; false: not colourable (more than 64
// colours, or an element with one row slot) — the row gather runs instead
bool ensure_colour(mfea_handle* h, Part& pt) {
  if (pt.ec_state) return pt.ec_state > 0;
  pt.ec_state = -1;
  if (!build_elem_colour(pt.P, pt.ec).empty()) return false;
  if (pt.ec.entry.empty() && pt.P.n_elems) return false;
  // (two buffers of their own; pt's sources; the assembly that reads them follows on the stream: no wait)
  if (pt.ec_entry.alloc(std::max<size_t>(pt.ec.entry.size(), 1)) != hipSuccess ||
      pt.ec_pos.alloc(std::max<size_t>(pt.ec.pos.size(), 1)) != hipSuccess ||
      h2d_async(h, pt.ec_entry.ptr, pt.ec.entry.data(), pt.ec.entry.size() * sizeof(int32_t)) != hipSuccess ||
      h2d_async(h, pt.ec_pos.ptr, pt.ec.pos.data(), pt.ec.pos.size() * sizeof(int32_t)) != hipSuccess)
    return false;
  pt.ec_state = 1;
  return true;
}

int assemble_impl(mfea_handle* h, mfea_stats* st, const double* rhs_dy = nullptr) {
  hipStream_t s = h->stream;
  RC(ensure_load_mask(h));  // (a no-op inside a step: step_impl has called it)
  h->assembled = true;
  h->rhs_fused = false;
  k_written(h);
  RC(phase_event(h, h->ev[0], s));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Pattern& P = pt.P;
    if (h->opt_asm_kernel == 1 && ensure_colour(h, pt)) {
      launch_assemble_colour(s, pt.ec.colors, pt.ec.cstart.data(), pt.ec_entry.ptr, pt.e2n_d.ptr, pt.ec_pos.ptr,
                             pt.xyz_d.ptr, pt.active.ptr, h->mat, pt.G, P.n_nodes, pt.val.ptr, pt.diag.ptr, h->sec_d());
      continue;  // (RHS: its own kernel in the solve, rhs_fused stays false)
    }
    if (h->opt_asm_kernel == 2 && ensure_colour(h, pt)) {
      launch_assemble_elems(s, P.n_elems, P.n_nodes, pt.e2n_d.ptr, pt.ec_pos.ptr, pt.xyz_d.ptr, pt.active.ptr,
                            h->mat, pt.slice_ptr.ptr, pt.row_len.ptr, pt.G, pt.val.ptr, pt.diag.ptr, h->sec_d());
      continue;
    }
    AsmRhs q{};
    const bool rhs = rhs_dy && h->parts.size() == 1;  // (rhs_dy: a one-partition GAMG / SOR / ICC step)
    if (rhs) {
      q = asm_rhs(h, pt, rhs_dy, nullptr);
      h->rhs_fused = true;
      h->rhs_dy[0] = rhs_dy[0];
      h->rhs_dy[1] = rhs_dy[1];
    }
    launch_assemble(s, P.n_nodes, pt.xyz_d.ptr, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr,
                    pt.s_elem.ptr, pt.active.ptr, h->mat, pt.G, pt.val.ptr, pt.diag.ptr, rhs ? &q : nullptr,
                    h->sec_d());
  }
  HIPC(hipGetLastError());
  RC(phase_event(h, h->ev[1], s));
  if (st && h->opt_phase_times) {
    RC(wait_event(h, h->ev[1]));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
    st->t_assemble_ms = ms;
  }
  return 0;
}

// Partitioned: the owned elements that failed in the last post (every
// partition's device list), as global ids, gathered from every rank, cleared
// in the host's global activity.  Over RCCL two all-gathers — the counts,
// then the lists padded to the longest — instead of the E-byte max-reduction
// of the whole activity (C5: 7 MB per failure step per rank).
int apply_failures(mfea_handle* h) {
  std::vector<int32_t> ids;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    unsigned c = 0;
    HIPC(hmemcpy(h, &c, pt.fail_cnt.ptr, sizeof c, hipMemcpyDeviceToHost));
    if (c > (unsigned)pt.P.n_elems) return fail(MFEA_EINVAL, "internal: failed-element list overflow");
    std::vector<int32_t> l(c);
    if (c) HIPC(hmemcpy(h, l.data(), pt.fail_list.ptr, c * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t le : l) ids.push_back((int32_t)pt.plan.elem_g[le]);
  }
  if (h->world > 1) {
    hipStream_t s = h->stream;
    const int W = h->world;
    HIPC(h->gfail.alloc(2 * (size_t)W));
    int32_t n = (int32_t)ids.size();
    HIPC(hipMemcpyAsync(h->gfail.ptr + h->rank, &n, sizeof n, hipMemcpyHostToDevice, s));
    NCCLC(ncclAllGather(h->gfail.ptr + h->rank, h->gfail.ptr + W, 1, ncclInt32, h->comm, s));
    std::vector<int32_t> cnt(W);
    HIPC(hipMemcpyAsync(cnt.data(), h->gfail.ptr + W, W * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RC(sync_stream(h));
    const int32_t mx = *std::max_element(cnt.begin(), cnt.end());
    if (mx > 0) {
      HIPC(h->gfail.alloc((size_t)(W + 1) * mx));
      std::vector<int32_t> mine(mx, -1);
      std::copy(ids.begin(), ids.end(), mine.begin());
      HIPC(hipMemcpyAsync(h->gfail.ptr, mine.data(), mx * sizeof(int32_t), hipMemcpyHostToDevice, s));
      NCCLC(ncclAllGather(h->gfail.ptr, h->gfail.ptr + mx, (size_t)mx, ncclInt32, h->comm, s));
      std::vector<int32_t> all((size_t)W * mx);
      HIPC(hipMemcpyAsync(all.data(), h->gfail.ptr + mx, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      RC(sync_stream(h));
      ids.clear();
      for (int r = 0; r < W; ++r)
        for (int32_t k = 0; k < cnt[r]; ++k) ids.push_back(all[(size_t)r * mx + k]);
    } else {
      ids.clear();
    }
  }
  for (int32_t g : ids) {
    if (g < 0 || g >= h->Ecount) return fail(MFEA_EINVAL, "internal: failed element id out of range");
    h->gkey[g] = 0;
  }
  return 0;
}

// One partition: the elements that failed in the last post (the stress
// kernel's list) move the host activity — O(failures), no E-byte copy or
// O(E) pass (src/fea_solver.py:283-284: elements only ever fail).  The
// list's counter is cleared for the next post.
unsigned* fail_counter(Part& pt) { return reinterpret_cast<unsigned*>(pt.red.ptr + 6); }

int local_failures(mfea_handle* h, Part& pt, unsigned c) {
  HostLap clk;
  if (c > (unsigned)pt.P.n_elems) return fail(MFEA_EINVAL, "internal: failed-element list overflow");
  std::vector<int32_t> ids(c);
  HIPC(hmemcpy(h, ids.data(), pt.fail_list.ptr, c * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPC(hipMemsetAsync(fail_counter(pt), 0, sizeof(unsigned), h->stream));
  if (!h->act_host_ok || h->act_host.size() != (size_t)pt.P.n_elems) return 0;
  for (int32_t e : ids) {
    if (e < 0 || e >= pt.P.n_elems || !h->act_host[e]) return fail(MFEA_EINVAL, "internal: bad failed element");
    h->act_host[e] = 0;
  }
  h->act_count -= (int64_t)c;
  clk.lap("failed ids", (int64_t)c);
  if (h->act_count != h->n_active) h->act_host_ok = false;  // cannot happen: fall back to a download
  return 0;
}

// the post kernels (reaction, stress / failures) and the read-back of their
// sums into h_red, ev[5] behind them
int enqueue_post_work(mfea_handle* h, double max_strain);
// The generalised force of the band of known rows [row0, row0 + nrows) into
// *out by the grip form, one launch on the post's partials and ticket set: a
// grip field Σ d·f of the band's rows; directions the band's reaction vector
// into sums[0..2] and its product with dir; the tensile test the y sum.
static void launch_band_force(hipStream_t s, Part& pt, const BcForm& bc, int64_t row0, int64_t nrows,
                              const double* dir, double* sums, double* out) {
  const Pattern& P = pt.P;
  with_grip(bc, [&](auto g) {
    using GM = decltype(g);
    if constexpr (std::is_same<GM, GripField>::value)
      launch_reaction_field(s, row0, nrows, P.n_nodes, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr, pt.val.ptr,
                            pt.diag.ptr, pt.G, pt.x.ptr, pt.partials.ptr, tix(pt, 3), out,
                            g.d + 3 * (row0 - P.n_free));
    else if constexpr (std::is_same<GM, GripVec>::value)
      launch_reaction3(s, row0, nrows, P.n_nodes, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr, pt.val.ptr,
                       pt.diag.ptr, pt.G, pt.x.ptr, pt.partials.ptr, tix(pt, 3), sums, dir, out);
    else
      launch_reaction(s, row0, nrows, P.n_nodes, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr, pt.val.ptr,
                      pt.diag.ptr, pt.G, pt.x.ptr, pt.partials.ptr, tix(pt, 3), out);
  });
}

int enqueue_post(mfea_handle* h, double max_strain) {
  RC(phase_event(h, h->ev[4], h->stream));
  RC(enqueue_post_work(h, max_strain));
  HIPC(hipEventRecord(h->ev[5], h->stream));
  return 0;
}
// the post's kernels and the read-back of their sums into the pinned h_red
// (capturable: the batch graph holds them)
int enqueue_event_work(mfea_handle* h);
int enqueue_post_work(mfea_handle* h, double max_strain) {
  if (h->ev_on) return enqueue_event_work(h);
  hipStream_t s = h->stream;
  const bool dm = partitioned(h);
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Pattern& P = pt.P;
    // (other directions than the tensile test's: the reaction vector of the
    // top rows into red[9..11] and the work-conjugate force into red[4], one launch)
    // (a grip field: the generalised force Σ d·f of the top rows into red[4])
    launch_band_force(s, pt, h->bc.form(pt), P.n_free, P.n_top, h->bc.grip.top, pt.red.ptr + 9, pt.red.ptr + 4);
    if (dm) HIPC(hipMemsetAsync(pt.fail_cnt.ptr, 0, sizeof(unsigned), s));
    // one partition: the counter is red[6] (read back with the force and the
    // count, no copy of its own), zero here — cleared by the host after the
    // last failures were read (local_failures)
    launch_stress(s, P.n_elems, pt.e2n_d.ptr, pt.xyz_d.ptr, pt.x.ptr, h->mat, max_strain,
                  pt.active.ptr, pt.stress.ptr, pt.partials.ptr, tix(pt, 4), pt.red.ptr + 5,
                  dm ? pt.elem_own.ptr : nullptr, pt.fail_list.ptr, dm ? pt.fail_cnt.ptr : fail_counter(pt),
                  h->Ee_d(), h->strength_d());
  }
  HIPC(hipGetLastError());
  Part& p0 = part0(h);
  if (dm) {  // (force, #active) of every partition, summed in rank order
    RC(gather4(h, 4));
    launch_rank_sum(s, p0.gred, nranks(h), p0.red.ptr + 12);
    HIPC(hipMemcpyAsync(h->h_red, p0.red.ptr + 12, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  } else {
    HIPC(hipMemcpyAsync(h->h_red, p0.red.ptr + 4, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  return 0;
}

// The post of an event (mfea_event; one partition): the scan — reaction and
// strains, one launch — then the apply, which reads the scan's maximum from
// device memory; then the read-back of F₁, #active, the failure counter, smax
// and lam (red[4..8]) into h_red[0..4].  Same tickets, failed-element list and
// counter as the plain post, so post_impl's bookkeeping serves both.
int enqueue_event_work(mfea_handle* h) {
  hipStream_t s = h->stream;
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  const bool vec = !h->bc.grip_default() && !h->bc.field.set;
  if ((int64_t)pt.partials.n < event_scan_partials(P.n_top, P.n_elems, vec))
    return fail(MFEA_EINVAL, "internal: partials too small for the event scan");
  double* eps = h->opt_event_scratch ? pt.eps.ptr : nullptr;
  EventScan q{};
  q.row0 = P.n_free;
  q.nrows = P.n_top;
  q.N = P.n_nodes;
  q.slice_ptr = pt.slice_ptr.ptr;
  q.row_len = pt.row_len.ptr;
  q.s_col = pt.s_col.ptr;
  q.val = pt.val.ptr;
  q.diag = pt.diag.ptr;
  q.G = pt.G;
  q.u = pt.x.ptr;
  q.partials = pt.partials.ptr;
  q.ticket_r = tix(pt, 3);
  q.force_out = pt.red.ptr + 4;
  q.E = P.n_elems;
  q.e2n = pt.e2n_d.ptr;
  q.xyz = pt.xyz_d.ptr;
  q.active = pt.active.ptr;
  q.eps = eps;
  q.ticket_e = tix(pt, 4);
  q.cnt_out = pt.red.ptr + 5;
  q.smax_out = pt.red.ptr + 7;
  q.strength = h->strength_d();
  q.vec = vec;
  for (int c = 0; c < 3; ++c) q.w[c] = h->bc.grip.top[c];
  q.sums = pt.red.ptr + 9;
  q.field = h->bc.form(pt).field;  // (the top rows are the first known rows)
  launch_event_scan(s, q);
  EventApply a{};
  a.E = P.n_elems;
  a.e2n = pt.e2n_d.ptr;
  a.xyz = pt.xyz_d.ptr;
  a.u = pt.x.ptr;
  a.eps = eps;
  a.Emod = h->mat.E;
  a.max_strain = h->ev_strain;
  a.tie_rtol = h->ev_tie;
  a.lam_max = h->ev_lam_max;
  a.k = h->ev_index;
  a.smax = pt.red.ptr + 7;
  a.active = pt.active.ptr;
  a.stress = pt.stress.ptr;
  a.event_of = pt.event_of.ptr;
  a.fail_list = pt.fail_list.ptr;
  a.fail_cnt = fail_counter(pt);
  a.partials = pt.partials.ptr;
  a.ticket = tix(pt, 4);
  a.cnt_out = pt.red.ptr + 5;
  a.lam_out = pt.red.ptr + 8;
  a.Ee = h->Ee_d();
  a.strength = h->strength_d();
  launch_event_apply(s, a);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h->h_red, pt.red.ptr + 4, 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  return 0;
}

// Speculative post (mfea_handle::spec_on), enqueued behind the solve's
// planned batch: the solve's end event, then the post.  At any later batch
// end the solve went on: that post's failures are undone and post runs after
// the solve's wait as usual
int spec_post(mfea_handle* h) {
  if (!h->spec_on) return 0;
  // a later batch end (the planned batch was not the last: SOR / ICC chunks,
  // a first solve): undo, and let post run after the solve as usual
  if (h->spec_used) return spec_undo(h);
  h->spec_used = true;
  RC(phase_event(h, h->ev[3], h->stream));
  RC(enqueue_post(h, h->spec_strain));
  h->spec_launched = true;
  return 0;
}
// the solve did not end with that batch's state: undo its post's failures
int spec_undo(mfea_handle* h) {
  if (!h->spec_launched) return 0;
  Part& pt = part0(h);
  if (h->ev_on) launch_event_unfail(h->stream, pt.fail_list.ptr, fail_counter(pt), pt.active.ptr, pt.event_of.ptr);
  else launch_unfail(h->stream, pt.fail_list.ptr, fail_counter(pt), pt.active.ptr);
  HIPC(hipGetLastError());
  h->spec_launched = false;
  return 0;
}

int post_impl(mfea_handle* h, double max_strain, double* total_force, int64_t* n_active,
              mfea_stats* st) {
  const bool dm = partitioned(h);
  if (!h->spec_launched) RC(enqueue_post(h, max_strain));
  h->spec_launched = false;
  Part& p0 = part0(h);
  RC(wait_event(h, h->ev[5]));
  if (!dm && p0.P.n_top == 0) h->h_red[0] = 0.0;
  if (!dm && p0.P.n_elems == 0) h->h_red[1] = 0.0;
  if (total_force) *total_force = h->h_red[0];
  unsigned nfail = 0;  // one partition: the stress kernel's failed-element count
  if (!dm) std::memcpy(&nfail, &h->h_red[2], sizeof nfail);
  // elements only ever fail here
  const bool changed = (int64_t)h->h_red[1] != h->n_active || nfail > 0;
  if (changed) {
    // every rank sees the same global count, so every rank exchanges
    if (dm && h->gkey_gen == h->act_gen) {
      RC(apply_failures(h));
      h->gkey_gen = h->act_gen + 1;
    }
    ++h->act_gen;
  }
  if ((int64_t)h->h_red[1] < h->Ecount) h->act_all = false;
  h->n_active = (int64_t)h->h_red[1];
  if (n_active) *n_active = h->n_active;
  if (!dm && nfail) RC(local_failures(h, p0, nfail));
  else if (!dm && h->act_host_ok && h->n_active != h->act_count) h->act_host_ok = false;
  if (st && h->opt_phase_times) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[4], h->ev[5]);
    st->t_post_ms = ms;
  }
  return 0;
}

// Partitioned GAMG: option "amg_dist" 1 the distributed V-cycle of the
// global hierarchy, 0 block Jacobi over per-partition hierarchies, -1 (the
// default) whichever solved faster: per active set the first solve runs the
// global hierarchy, the second block Jacobi (plan builds and uploads outside
// the clock), later ones the faster of the two.  The block-Jacobi form wins
// where the partition boundaries cut weak couplings (strips between tiles:
// the same iteration count with two exchanges per iteration instead of
// 4·levels + 2); the global form wherever the cut couplings matter (the
// grown networks: 17 iterations instead of 190-310).  A variant that fails
// (max_it, breakdown) hands the step to the other.
// RCCL world: *t ← the maximum of *t over the ranks (collective)
int max_over_ranks(mfea_handle* h, double* t) {
  HIPC(h->gtime.alloc(1));
  HIPC(hipMemcpyAsync(h->gtime.ptr, t, sizeof(double), hipMemcpyHostToDevice, h->stream));
  NCCLC(ncclAllReduce(h->gtime.ptr, h->gtime.ptr, 1, ncclFloat64, ncclMax, h->comm, h->stream));
  HIPC(hipMemcpyAsync(t, h->gtime.ptr, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sync_stream(h);
}

int solve_amg_part(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o, mfea_stats* st) {
  auto run = [&](int mode) {
    return mode ? solve_gamg_global(h, dy_top, dy_bot, o, st) : solve_amg_dist(h, dy_top, dy_bot, o, st);
  };
  if (h->opt_amg_dist >= 0) return run(h->opt_amg_dist);
  auto& a = h->amg_auto;
  bool rebuilt = false;
  RC(ensure_gamg_plan(h, &rebuilt));  // the active set's identity (a content compare)
  if (a.gen != h->gamg_plan_gen) {
    a.gen = h->gamg_plan_gen;
    a.choice = -1;
    a.t[0] = a.t[1] = -1.0;
  }
  if (a.choice >= 0) return run(a.choice);
  const int mode = amg_auto_pending(a.t);
  if (mode) {
    RC(ensure_gamg(h, &rebuilt));
  } else {
    for (auto& pp : h->parts) {
      bool rb = false;
      RC(ensure_amg(h, *pp, &rb));
      rebuilt = rebuilt || rb;
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  int rc = run(mode);
  if (rc == 0) rc = sync_stream(h);
  a.t[mode] = rc == 0 ? std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() : 1e300;
  // RCCL: every rank must pick the same form (the two issue different
  // exchanges), so each compares the slowest rank's times, not its own
  if (h->world > 1) RC(max_over_ranks(h, &a.t[mode]));
  if (amg_auto_pending(a.t) < 0) a.choice = amg_auto_choice(a.t);
  if (rc == MFEA_EMAXIT || rc == MFEA_EBREAKDOWN) {
    a.choice = 1 - mode;
    rc = run(a.choice);
  }
  if (st && rebuilt) st->amg_rebuilt = 1;
  return rc;
}

int solve_any(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* o,
              mfea_stats* st) {
  h->ev_setup_used = false;
  h->setup_skipped = false;
  h->bc.load_dy_top = dy_top;  // (mfea_get_load_work: the amplitude of the last solve)
  // another preconditioner kind than the last solve's: its setup runs
  if (o->precond != h->last_precond) drop_kept_setup(h);
  h->last_precond = o->precond;
  if (o->precond == MFEA_PC_GAMG) {
    if (!partitioned(h)) return solve_amg(h, dy_top, dy_bot, o, st);
    return solve_amg_part(h, dy_top, dy_bot, o, st);
  }
  if (o->precond == MFEA_PC_SOR || o->precond == MFEA_PC_ICC) {
    if (partitioned(h)) return fail(MFEA_EINVAL, "MFEA_PC_SOR / MFEA_PC_ICC: one partition per handle");
    return solve_amg(h, dy_top, dy_bot, o, st);
  }
  if (o->precond != MFEA_PC_JACOBI && o->precond != MFEA_PC_BLOCK_JACOBI)
    return fail(MFEA_EINVAL, "unknown preconditioner");
  return partitioned(h) ? solve_dist(h, dy_top, dy_bot, o, st) : solve_impl(h, dy_top, dy_bot, o, st);
}

// current element activity in original order (elements no partition of this
// process holds stay 1)
int gather_active(mfea_handle* h, std::vector<uint8_t>& out) {
  out.assign(h->Ecount, 1);
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int64_t E = pt.P.n_elems;
    std::vector<uint8_t> a(E);
    if (E) HIPC(hmemcpy(h, a.data(), pt.active.ptr, E, hipMemcpyDeviceToHost));
    if (!partitioned(h)) {
      out = a;
      return 0;
    }
    for (int64_t le = 0; le < E; ++le) out[pt.plan.elem_g[le]] = a[le];
  }
  return 0;
}

}  // namespace

extern "C" {

int mfea_abi_version(void) { return MFEA_ABI_VERSION; }

int mfea_last_error(char* buf, size_t n) {
  if (!buf || n == 0) return MFEA_EINVAL;
  std::snprintf(buf, n, "%s", g_err.c_str());
  return 0;
}

int mfea_create(int device, mfea_handle** out) {
  if (!out) return fail(MFEA_EINVAL, "out is NULL");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return fail(MFEA_EDEVICE, "no HIP device available");
  if (device < 0 || device >= count) return fail(MFEA_EINVAL, "device index out of range");
  auto* h = new mfea_handle();
  h->device = device;
  HIPC(hipSetDevice(device));
  HIPC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (auto& ev : h->ev) HIPC(hipEventCreate(&ev));
  HIPC(hipEventCreate(&h->ev_setup));
  for (auto& ev : h->poll) HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPC(hipHostMalloc(&h->h_state, 2 * sizeof(SolveState),
                     hipHostMallocMapped | hipHostMallocCoherent));
  HIPC(hipHostGetDevicePointer((void**)&h->d_host_state, h->h_state, 0));
  HIPC(hipHostMalloc(&h->h_red, 16 * sizeof(double), hipHostMallocDefault));
  std::memset(h->h_state, 0, 2 * sizeof(SolveState));
  h->parts.push_back(std::make_unique<Part>());  // scratch of mfea_solve_csr until a mesh is set
  h->parts[0]->mirror = h->d_host_state;
  // reference constants src/fea_solver.py:14-20
  const double d = 0.0002, t = 0.000001;
  const double A = 3.14 * (std::pow(d / 2, 2) - std::pow(d / 2 - t, 2));
  mfea_set_material(h, 2500.0, A, A * 0.001);
  *out = h;
  return 0;
}

int mfea_destroy(mfea_handle* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  destroy_graph(h);
  for (auto& g : h->graph_setup)
    if (g) (void)hipGraphExecDestroy(g);
  for (auto& form : h->graph_combo)
    for (auto& g : form)
      if (g) (void)hipGraphExecDestroy(g);
  h->parts.clear();
  if (h->comm) (void)ncclCommDestroy(h->comm);
  for (auto& ev : h->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : h->poll)
    if (ev) (void)hipEventDestroy(ev);
  if (h->ev_setup) (void)hipEventDestroy(h->ev_setup);
  if (h->h_state) (void)hipHostFree(h->h_state);
  if (h->h_red) (void)hipHostFree(h->h_red);
  if (h->run_copy) {
    (void)hipStreamSynchronize(h->run_copy);
    (void)hipStreamDestroy(h->run_copy);
  }
  for (int i = 0; i < 2; ++i) {
    if (h->run_ready[i]) (void)hipEventDestroy(h->run_ready[i]);
    if (h->run_free[i]) (void)hipEventDestroy(h->run_free[i]);
    if (h->run_pin[i]) (void)hipHostFree(h->run_pin[i]);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int mfea_set_material(mfea_handle* h, double E, double A, double I) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  h->E = E;
  h->A = A;
  h->I = I;
  h->mat.EA = E * A;             // src/fea_solver.py:45  (E * A) / L_safe
  h->mat.EI12 = (12.0 * E) * I;  // src/fea_solver.py:58  12 * E * I / L³
  h->mat.E = E;
  // K and everything formed from it are the old material's: the next step
  // assembles (k_current compares the material by value) and sets up; the
  // graphs that hold the material by value are keyed by it (graph_batch_mat,
  // the combined graph's key)
  ++h->op_gen;
  // per-element columns stay; the columns left to the scalars follow them
  if (h->has_props()) {
    RC(set_device(h));
    RC(upload_props(h));
  }
  return 0;
}

// The directions enter the right-hand side, the prescribed rows of x and the
// reaction only: K, the symbolic hierarchy and the kept values stay.  What
// holds the old vectors goes: the RHS mfea_step's assembly cached, and every
// captured graph (the step head and the post hold the vectors and the
// kernels' GripY / GripVec form by value) — the stream is drained first, so
// none is in flight.  A z component on a planar mesh changes the lane layout
// (lane_dofs): the rebuild a layout option takes, the activity kept.
// (nd0: lane_dofs before the change)
static int grip_changed(mfea_handle* h, int nd0) {
  h->rhs_fused = false;
  destroy_graph(h);
  for (auto& gs : h->graph_setup) {
    if (gs) (void)hipGraphExecDestroy(gs);
    gs = nullptr;
  }
  for (auto& form : h->graph_combo)
    for (auto& gc : form) {
      if (gc) (void)hipGraphExecDestroy(gc);
      gc = nullptr;
    }
  if (lane_dofs(h) != nd0) {
    if (!h->dirty && h->has_mesh && h->Ecount) RC(gather_active(h, h->active_host));
    h->dirty = true;
  }
  return 0;
}

// The shared middle of mfea_set_grip_field and mfea_set_node_loads, behind
// their checks: the stream drained, then staged (stage_node_vectors) made the
// state of nv.  *nd0: lane_dofs before the change, for grip_changed.
static int swap_node_vectors(mfea_handle* h, NodeVectors& nv, std::vector<double>& staged, bool set, int* nd0) {
  RC(set_device(h));
  *nd0 = lane_dofs(h);
  if (h->stream) HIPC(hipStreamSynchronize(h->stream));
  nv.v.swap(staged);
  nv.set = set;
  return 0;
}

int mfea_set_grip_motion(mfea_handle* h, const double top[3], const double bot[3]) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  // (what the next build will be decides, not the partitions a handle still
  // holds from before mfea_debug_set_parts(h, 1): those wait for the rebuild)
  if (h->world > 1 || h->nparts > 1) return fail(MFEA_ESTATE, "mfea_set_grip_motion: one partition per handle");
  for (const double* v : {top, bot}) {
    if (!v) continue;
    if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2]))
      return fail(MFEA_EINVAL, "mfea_set_grip_motion: every component must be finite");
    if (v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0)
      return fail(MFEA_EINVAL, "mfea_set_grip_motion: a direction must not be all zero");
  }
  GripVec g = h->bc.grip;
  for (int c = 0; c < 3; ++c) {
    // (+ 0.0: a −0 component is stored as 0 — dy · 0 has the sign of dy either way)
    if (top) g.top[c] = top[c] + 0.0;
    if (bot) g.bot[c] = bot[c] + 0.0;
  }
  if (std::memcmp(&g, &h->bc.grip, sizeof g) == 0) return 0;
  RC(set_device(h));
  const int nd0 = lane_dofs(h);
  if (h->stream) HIPC(hipStreamSynchronize(h->stream));
  h->bc.grip = g;
  return grip_changed(h, nd0);
}

// A vector per grip node in place of the band's direction: it enters where the
// directions enter and a change drops what a change of them drops
// (grip_changed).  The host copy is the state; the device rows are gathered
// from it here, when the handle is built, and at every build.
int mfea_set_grip_field(mfea_handle* h, const double* field) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "set the mesh before the grip field");
  if (h->world > 1 || h->nparts > 1) return fail(MFEA_ESTATE, "mfea_set_grip_field: one partition per handle");
  std::vector<double> f;
  const VecStage st = stage_node_vectors(h->bc.field, field, (size_t)3 * h->N, f);
  if (st == VecStage::kNotFinite) return fail(MFEA_EINVAL, "mfea_set_grip_field: every entry must be finite");
  if (st == VecStage::kSame) return 0;
  int nd0 = 0;
  RC(swap_node_vectors(h, h->bc.field, f, field != nullptr, &nd0));
  RC(grip_changed(h, nd0));
  if (h->bc.field.set && !h->dirty && h->parts.size() == 1) RC(upload_field(h, part0(h)));
  return 0;
}

int mfea_get_grip_field(mfea_handle* h, double* field, int32_t* is_set) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "no mesh: call mfea_set_mesh first");
  if (is_set) *is_set = h->bc.field.set ? 1 : 0;
  if (!field) return 0;
  if (h->bc.field.set) {
    std::copy(h->bc.field.v.begin(), h->bc.field.v.end(), field);
    return 0;
  }
  std::fill(field, field + 3 * h->N, 0.0);
  for (const int64_t n : h->top)
    for (int c = 0; c < 3; ++c) field[3 * n + c] = h->bc.grip.top[c];
  for (const int64_t n : h->bot)
    for (int c = 0; c < 3; ++c) field[3 * n + c] = h->bc.grip.bot[c];
  return 0;
}

int mfea_get_grip_motion(mfea_handle* h, double top[3], double bot[3]) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  for (int c = 0; c < 3; ++c) {
    if (top) top[c] = h->bc.grip.top[c];
    if (bot) bot[c] = h->bc.grip.bot[c];
  }
  return 0;
}

int mfea_get_reaction(mfea_handle* h, double top[3], double bot[3]) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_get_reaction: one partition per handle");
  if (!h->assembled) return fail(MFEA_ESTATE, "mfea_get_reaction: no assembly since the last build");
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  hipStream_t s = h->stream;
  // the two bands are contiguous row ranges: top [n_free, n_free + n_top),
  // bottom from there to the ghost rows; sums into red[9..11] and red[12..14]
  const int64_t row0[2] = {P.n_free, P.n_free + P.n_top};
  const int64_t nrows[2] = {P.n_top, P.n_nodes - P.n_ghost - P.n_free - P.n_top};
  double* const out[2] = {top, bot};
  for (int b = 0; b < 2; ++b) {
    if (!out[b]) continue;
    launch_reaction3(s, row0[b], nrows[b], P.n_nodes, pt.slice_ptr.ptr, pt.row_len.ptr, pt.s_col.ptr, pt.val.ptr,
                     pt.diag.ptr, pt.G, pt.x.ptr, pt.partials.ptr, tix(pt, 3), pt.red.ptr + 9 + 3 * b, nullptr,
                     nullptr);
    HIPC(hipGetLastError());
    HIPC(hmemcpy(h, out[b], pt.red.ptr + 9 + 3 * b, 3 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}

// The generalised force of each band (states and launches as mfea_get_reaction):
// under a grip field Σ d·f of the band's rows, one launch per band; without,
// the band's reaction vector and its product with the band's direction — the
// post's launch and, for the top band, its bits.  Outputs in a buffer of the
// call's own; the post's partials and ticket set, behind the post on the stream.
int mfea_get_grip_work(mfea_handle* h, double* top, double* bot) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_get_grip_work: one partition per handle");
  if (!h->assembled) return fail(MFEA_ESTATE, "mfea_get_grip_work: no assembly since the last build");
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  hipStream_t s = h->stream;
  HIPC(pt.gw_red.alloc(4));
  const int64_t row0[2] = {P.n_free, P.n_free + P.n_top};
  const int64_t nrows[2] = {P.n_top, P.n_nodes - P.n_ghost - P.n_free - P.n_top};
  const double* const dir[2] = {h->bc.grip.top, h->bc.grip.bot};
  double* const out[2] = {top, bot};
  BcForm bc = h->bc.form(pt);
  bc.grip = &h->bc.grip;  // (the reaction vector and its product for the tensile directions too)
  for (int b = 0; b < 2; ++b) {
    if (!out[b]) continue;
    launch_band_force(s, pt, bc, row0[b], nrows[b], dir[b], pt.gw_red.ptr, pt.gw_red.ptr + 3);
    HIPC(hipGetLastError());
    HIPC(hmemcpy(h, out[b], pt.gw_red.ptr + 3, sizeof(double), hipMemcpyDeviceToHost));
  }
  return 0;
}

// A force vector per free node (bc_form.hpp NodeLoad): it enters where the
// grips' values enter, the four RHS sites, and a change drops what a change of
// them drops (grip_changed).  The host copy is the state; the device rows are
// gathered from it here, when the handle is built, and at every build.
int mfea_set_node_loads(mfea_handle* h, const double* loads, int32_t mode) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "set the mesh before the nodal loads");
  if (h->world > 1 || h->nparts > 1) return fail(MFEA_ESTATE, "mfea_set_node_loads: one partition per handle");
  if (loads && mode != MFEA_LOAD_DEAD && mode != MFEA_LOAD_PROPORTIONAL)
    return fail(MFEA_EINVAL, "mfea_set_node_loads: mode must be MFEA_LOAD_DEAD or MFEA_LOAD_PROPORTIONAL");
  std::vector<double> f;
  const VecStage st = stage_node_vectors(h->bc.loads, loads, (size_t)3 * h->N, f);
  if (st == VecStage::kNotFinite) return fail(MFEA_EINVAL, "mfea_set_node_loads: every entry must be finite");
  if (st == VecStage::kSame && (!loads || h->bc.load_mode == mode)) return 0;
  int nd0 = 0;
  RC(swap_node_vectors(h, h->bc.loads, f, loads != nullptr, &nd0));
  h->bc.load_mode = loads ? mode : MFEA_LOAD_DEAD;
  RC(grip_changed(h, nd0));
  if (h->bc.loads.set && !h->dirty && h->parts.size() == 1) RC(upload_loads(h, part0(h)));
  return 0;
}

int mfea_get_node_loads(mfea_handle* h, double* loads, int32_t* mode, int32_t* is_set) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "no mesh: call mfea_set_mesh first");
  if (is_set) *is_set = h->bc.loads.set ? 1 : 0;
  if (mode) *mode = h->bc.load_mode;
  if (!loads) return 0;
  if (h->bc.loads.set) std::copy(h->bc.loads.v.begin(), h->bc.loads.v.end(), loads);
  else std::fill(loads, loads + 3 * h->N, 0.0);
  return 0;
}

// L = Σ q·u over the free, non-floating rows (kernels.hip k_load_work): the
// amplitude and the mask of the last solve, the current U; states as
// mfea_get_reaction.  The post's partials and ticket set, behind the post on
// the stream; the output in a buffer of the call's own.
int mfea_get_load_work(mfea_handle* h, double* work) {
  if (!h || !work) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_get_load_work: one partition per handle");
  if (!h->assembled) return fail(MFEA_ESTATE, "mfea_get_load_work: no assembly since the last build");
  *work = 0.0;
  if (!h->bc.loads.set) return 0;
  Part& pt = part0(h);
  HIPC(pt.lw_red.alloc(1));
  launch_load_work(h->stream, pt.P.n_free, pt.ld, h->bc.load_dy_top, pt.x.ptr, pt.partials.ptr, tix(pt, 3),
                   pt.lw_red.ptr);
  HIPC(hipGetLastError());
  HIPC(hmemcpy(h, work, pt.lw_red.ptr, sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// The strain energy of every element that counts and its two parts per unit
// section (kernels.hip k_energy), on the handle's stream: behind everything
// earlier calls enqueued there — a speculative post's undo included — so the
// displacement and the activity it reads are the ones the getters return.  It
// writes buffers of its own only: no generation moves, nothing kept is dropped.
int mfea_get_energy(mfea_handle* h, const double* U, const uint8_t* active, double total[2],
                    const mfea_element_energy* out) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "no mesh: call mfea_set_mesh first");
  if (h->world > 1 || h->nparts > 1 || h->parts.size() > 1)
    return fail(MFEA_ESTATE, "mfea_get_energy: one partition per handle");
  if (h->top.empty() && h->bot.empty())
    return fail(MFEA_ESTATE, "mfea_get_energy: no boundary conditions (mfea_set_bc)");
  RC(set_device(h));
  RC(ensure_built(h));
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  const int64_t N = P.n_nodes, E = P.n_elems;
  hipStream_t s = h->stream;
  double* const host[4] = {out ? out->w_axial : nullptr, out ? out->w_bending : nullptr,
                           out ? out->g_axial : nullptr, out ? out->g_bending : nullptr};
  int rows = 0;
  for (double* p : host) rows += p != nullptr;
  HIPC(pt.en_out.alloc((size_t)rows * E + 2));
  HIPC(pt.en_part.alloc((size_t)energy_partials(E)));
  if (U) HIPC(pt.en_u.alloc(3 * N));
  if (active) HIPC(pt.en_act.alloc(E));
  const bool first = !pt.en_tix.ptr;
  HIPC(pt.en_tix.alloc(kTicketStride));
  // a caller's U, original node order → row order, and a caller's mask; the
  // host sources live until the stream is waited for below, error or not
  // (hmemcpy's rule)
  std::vector<double> up;
  std::vector<uint8_t> am;
  if (U) {
    up.resize(3 * N);
    for (int64_t i = 0; i < N; ++i)
      for (int a = 0; a < 3; ++a) up[3 * i + a] = U[3 * P.perm[i] + a];
  }
  if (active) {
    am.resize(E);
    for (int64_t e = 0; e < E; ++e) am[e] = active[e] ? 1 : 0;
  }
  double* dev[4] = {nullptr, nullptr, nullptr, nullptr};
  double* next = pt.en_out.ptr;
  for (int k = 0; k < 4; ++k) {
    if (!host[k]) continue;
    dev[k] = next;
    next += E;
  }
  double* red = pt.en_out.ptr + (size_t)rows * E;
  double tot[2] = {0.0, 0.0};
  hipError_t e = first ? hipMemsetAsync(pt.en_tix.ptr, 0, kTicketStride * sizeof(unsigned), s) : hipSuccess;
  if (e == hipSuccess && U) e = h2d_async(h, pt.en_u.ptr, up.data(), up.size() * sizeof(double));
  if (e == hipSuccess && active) e = h2d_async(h, pt.en_act.ptr, am.data(), am.size());
  if (e == hipSuccess) {
    launch_energy(s, E, pt.e2n_d.ptr, pt.xyz_d.ptr, U ? pt.en_u.ptr : pt.x.ptr, active ? pt.en_act.ptr : pt.active.ptr,
                  h->mat, h->sec_d(), EnergyOut{dev[0], dev[1], dev[2], dev[3]}, pt.en_part.ptr, pt.en_tix.ptr, red);
    e = hipGetLastError();
  }
  for (int k = 0; k < 4 && e == hipSuccess; ++k)
    if (host[k] && E) e = hipMemcpyAsync(host[k], dev[k], E * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(tot, red, sizeof tot, hipMemcpyDeviceToHost, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (e != hipSuccess || es != hipSuccess)
    return fail(MFEA_EDEVICE, std::string("mfea_get_energy: ") + hipGetErrorString(e != hipSuccess ? e : es));
  if (total) {
    total[0] = tot[0];
    total[1] = tot[1];
  }
  return 0;
}

static bool props_column_ok(const double* v, int64_t n, bool strength) {
  for (int64_t e = 0; v && e < n; ++e) {
    if (strength ? !(v[e] > 0.0) : !(std::isfinite(v[e]) && v[e] >= 0.0)) return false;
  }
  return true;
}

int mfea_set_element_props(mfea_handle* h, const mfea_element_props* p) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "set the mesh before the element properties");
  if (h->world > 1 || h->nparts > 1 || h->parts.size() > 1)
    return fail(MFEA_ESTATE, "mfea_set_element_props: one partition per handle");
  const int64_t n = h->Ecount;
  const mfea_element_props none{nullptr, nullptr, nullptr, nullptr};
  if (!p) p = &none;
  if (!props_column_ok(p->E, n, false) || !props_column_ok(p->A, n, false) || !props_column_ok(p->I, n, false))
    return fail(MFEA_EINVAL, "mfea_set_element_props: E, A, I must be finite and >= 0");
  if (!props_column_ok(p->max_strain, n, true))
    return fail(MFEA_EINVAL, "mfea_set_element_props: max_strain must be > 0 (+inf allowed)");
  RC(set_device(h));
  auto take = [n](std::vector<double>& v, const double* src) {
    if (src && n > 0) v.assign(src, src + n);
    else v.clear();
  };
  take(h->pe_E, p->E);
  take(h->pe_A, p->A);
  take(h->pe_I, p->I);
  take(h->pe_S, p->max_strain);
  return upload_props(h);
}

int mfea_get_element_props(mfea_handle* h, double* E, double* A, double* I, double* max_strain) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "no mesh: call mfea_set_mesh first");
  const int64_t n = h->Ecount;
  auto give = [n](double* out, const std::vector<double>& v, double scalar) {
    if (!out) return;
    if (v.empty()) std::fill(out, out + n, scalar);
    else std::copy(v.begin(), v.end(), out);
  };
  give(E, h->pe_E, h->E);
  give(A, h->pe_A, h->A);
  give(I, h->pe_I, h->I);
  give(max_strain, h->pe_S, std::numeric_limits<double>::quiet_NaN());
  return 0;
}

int mfea_set_mesh(mfea_handle* h, int64_t n_nodes, const double* xyz, int64_t n_elems,
                  const int64_t* e2n, uint32_t flags) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (n_nodes < 0 || n_elems < 0) return fail(MFEA_EINVAL, "negative size");
  if ((n_nodes && !xyz) || (n_elems && !e2n)) return fail(MFEA_EINVAL, "NULL mesh array");
  RC(set_device(h));
  h->N = n_nodes;
  h->Ecount = n_elems;
  h->xyz.assign(xyz, xyz + 3 * n_nodes);
  h->e2n.assign(e2n, e2n + 2 * n_elems);
  h->mesh_flags = flags;
  h->has_mesh = true;
  h->dirty = true;
  h->act_all = false;
  h->active_host.clear();
  clear_props(h);  // (indexed by the old mesh's elements)
  // (... the nodal loads and the grip field by its nodes: cleared, as
  // mfea_set_node_loads(h, NULL, 0) and mfea_set_grip_field(h, NULL))
  for (NodeVectors* nv : {&h->bc.loads, &h->bc.field}) {
    if (!nv->set) continue;
    if (h->stream) HIPC(hipStreamSynchronize(h->stream));
    nv->reset();
    if (nv == &h->bc.loads) h->bc.load_mode = MFEA_LOAD_DEAD;
    RC(grip_changed(h, lane_dofs(h)));
  }
  h->planar = true;
  for (int64_t n = 0; n < n_nodes; ++n)
    if (xyz[3 * n + 2] != 0.0) h->planar = false;
  // validate now so errors surface at the call that caused them
  Pattern tmp;
  std::string err = build_pattern(h->N, h->xyz.data(), h->Ecount, h->e2n.data(),
                                  (flags & MFEA_MESH_SKIP_INVALID) != 0, {}, {}, 0, tmp);
  if (!err.empty()) {
    h->has_mesh = false;
    return fail(MFEA_EINVAL, err);
  }
  return 0;
}

int mfea_set_bc(mfea_handle* h, int64_t n_top, const int64_t* top, int64_t n_bot,
                const int64_t* bot) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (!h->has_mesh) return fail(MFEA_ESTATE, "set the mesh before the boundary conditions");
  if (n_top < 0 || n_bot < 0 || (n_top && !top) || (n_bot && !bot))
    return fail(MFEA_EINVAL, "bad grip node arrays");
  for (int64_t i = 0; i < n_top; ++i)
    if (top[i] < 0 || top[i] >= h->N) return fail(MFEA_EINVAL, "top grip node out of range");
  for (int64_t i = 0; i < n_bot; ++i)
    if (bot[i] < 0 || bot[i] >= h->N) return fail(MFEA_EINVAL, "bottom grip node out of range");
  // keep the current activity across the rebuild
  if (!h->dirty && h->Ecount) RC(gather_active(h, h->active_host));
  h->top.assign(top, top + n_top);
  h->bot.assign(bot, bot + n_bot);
  h->dirty = true;
  return 0;
}

int mfea_set_active(mfea_handle* h, const uint8_t* active) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  // all active already (the benchmark resets every step): nothing changes —
  // no act_gen bump, so a partitioned handle skips its activity all-reduce
  if (!active && h->act_all) return 0;
  ++h->act_gen;
  ++h->act_sub_gen;
  h->act_all = !active;
  if (partitioned(h)) {  // the global activity is known here: no exchange needed for it
    h->gkey.assign(h->Ecount, 1);
    if (active)
      for (int64_t e = 0; e < h->Ecount; ++e) h->gkey[e] = active[e] ? 1 : 0;
    h->gkey_gen = h->act_gen;
  }
  if (h->Ecount == 0) return 0;
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int64_t E = pt.P.n_elems;
    if (!E) continue;
    if (active) {
      std::vector<uint8_t> a(E);
      for (int64_t le = 0; le < E; ++le)
        a[le] = active[partitioned(h) ? pt.plan.elem_g[le] : le] ? 1 : 0;
      HIPC(hmemcpy(h, pt.active.ptr, a.data(), E, hipMemcpyHostToDevice));
      if (!partitioned(h)) h->act_host = std::move(a);
    } else {
      HIPC(hmemset(h, pt.active.ptr, 1, E));
      if (!partitioned(h)) h->act_host.assign(E, 1);
    }
  }
  if (!partitioned(h)) {
    h->act_count = (int64_t)std::count(h->act_host.begin(), h->act_host.end(), (uint8_t)1);
    h->act_host_ok = true;
    h->n_active = h->act_count;  // (as ensure_built)
  }
  return 0;
}

int mfea_assemble(mfea_handle* h) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  RC(assemble_impl(h, nullptr));
  return sync_stream(h);
}

int mfea_solve(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
               mfea_stats* st) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  mfea_solve_opts o = opts ? *opts : default_opts();
  if (st) std::memset(st, 0, sizeof(*st));
  // a (re)build (new mesh / BCs, a layout option) left the operator empty:
  // assemble the current active set first rather than solve a zero operator
  if (!h->assembled) RC(assemble_impl(h, nullptr));
  // (nodal loads set after the assembly: no mask of K's activity yet — the
  // current one's, which is K's unless a post has moved it since)
  if (h->bc.loads.set && !partitioned(h) && part0(h).ld_mask_gen != h->k_from.act_gen) RC(ensure_load_mask(h));
  return solve_any(h, dy_top, dy_bot, &o, st);
}

int mfea_post(mfea_handle* h, double max_strain, double* total_force, int64_t* n_active) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  return post_impl(h, max_strain, total_force, n_active, nullptr);
}

// mfea_step's body; h->ev_on: the post is the event pair (mfea_event)
static int step_impl(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
                     double max_strain, double* total_force, int64_t* n_active, mfea_stats* st) {
  mfea_solve_opts o = opts ? *opts : default_opts();
  if (st) std::memset(st, 0, sizeof(*st));
  // nodal loads: the floating mask of the activity this step's K is assembled
  // from, in front of every RHS of the step and outside its graphs
  RC(ensure_load_mask(h));
  // the one-partition GAMG / SOR / ICC solves take their RHS from the
  // assembly's row pass (AsmRhs)
  const bool fuse_rhs = !partitioned(h) && (o.precond == MFEA_PC_GAMG || o.precond == MFEA_PC_SOR ||
                                            o.precond == MFEA_PC_ICC);
  const double dys[2] = {dy_top, dy_bot};
  // one partition, GAMG / SOR / ICC, graphs on, no phase events, the row
  // gather: the assembly rides at the head of the solve's setup graph
  const bool defer = fuse_rhs && h->opt_step_graph && h->opt_graph && !h->opt_phase_times && h->opt_asm_kernel == 0;
  if (!partitioned(h) && k_current(h)) {
    // K is what this assembly would write (option keep_operator): only the
    // RHS depends on the grip displacements — the RHS-only kernel of
    // mfea_solve, between the assembly's phase events (the Jacobi kinds form
    // theirs in the solve)
    hipStream_t s = h->stream;
    ++h->op_kept_steps;
    h->rhs_fused = false;
    RC(phase_event(h, h->ev[0], s));
    // (GAMG with option amg_start: left to solve_amg, which knows whether the
    // hierarchy's values are kept too and then forms the RHS in k_amg_start —
    // the same kernel from there otherwise)
    if (fuse_rhs && !(h->opt_amg_start && o.precond == MFEA_PC_GAMG)) {
      Part& pt = part0(h);
      launch_cg_rhs(s, sell_op(pt), pt.code.ptr, dy_top, dy_bot, o.reg, 2, cg_vecs(pt), pt.partials.ptr, tix(pt, 0),
                    pt.red.ptr, h->bc.form(pt));
      HIPC(hipGetLastError());
      h->rhs_fused = true;
      h->rhs_dy[0] = dy_top;
      h->rhs_dy[1] = dy_bot;
    }
    RC(phase_event(h, h->ev[1], s));
  } else if (defer) {
    h->h_red[14] = dy_top;
    h->h_red[15] = dy_bot;
    h->asm_pending = true;
    h->assembled = true;
    h->rhs_fused = false;
  } else {
    RC(assemble_impl(h, nullptr, fuse_rhs ? dys : nullptr));
  }
  // a solver failure stops the step loop here, as the reference does
  // (src/fea_petsc.cpp:346-354)
  h->in_step = true;
  h->spec_on = fuse_rhs && h->opt_spec_post;
  h->spec_strain = max_strain;
  h->spec_launched = false;
  h->spec_used = false;
  int rc = solve_any(h, dy_top, dy_bot, &o, st);
  h->spec_on = false;
  h->rhs_fused = false;
  if (h->asm_pending) {  // (the solve ended before its assembly: never on success)
    h->asm_pending = false;
    if (rc == 0) rc = assemble_impl(h, nullptr);
    else h->assembled = false;
  }
  if (rc) (void)spec_undo(h);
  if (rc == 0) rc = post_impl(h, max_strain, total_force, n_active, st);
  h->in_step = false;
  if (rc) {
    drop_kept(h);  // (a failed step: the next one assembles and sets up)
    (void)sync_stream(h);
    return rc;
  }
  if (st && h->opt_phase_times) {  // every event of the step has completed (post waited)
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
    st->t_assemble_ms = ms;
    solve_times(h, st);
  }
  return 0;
}

int mfea_step(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
              double max_strain, double* total_force, int64_t* n_active, mfea_stats* st) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  return step_impl(h, dy_top, dy_bot, opts, max_strain, total_force, n_active, st);
}

// ---------------------------------------------------------------------------
// mfea_event: one step at the reference load whose post is the event pair.
// ---------------------------------------------------------------------------
// events scale one solve to each failure load: U must be proportional to the
// amplitudes, which a dead load breaks (the response is affine in the factor)
static const char kDeadLoadEvents[] =
    "events need a response proportional to the amplitudes: dead nodal loads make it affine in the load factor "
    "(mfea_set_node_loads with MFEA_LOAD_PROPORTIONAL, or NULL, first)";
static int event_check(const mfea_event_opts* ev) {
  if (!ev) return fail(MFEA_EINVAL, "NULL argument");
  if (!(ev->max_strain > 0.0)) return fail(MFEA_EINVAL, "mfea_event: max_strain must be > 0");
  if (!(ev->tie_rtol >= 0.0 && ev->tie_rtol < 1.0)) return fail(MFEA_EINVAL, "mfea_event: tie_rtol must be in [0, 1)");
  if (!(ev->lam_max > 0.0)) return fail(MFEA_EINVAL, "mfea_event: lam_max must be > 0 (+inf allowed)");
  return 0;
}

// event `index` of a run (0 for a single mfea_event) on a built one-partition handle
static int event_impl(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
                      const mfea_event_opts* ev, int32_t index, mfea_event_out* out, mfea_stats* st) {
  h->ev_strain = ev->max_strain;
  h->ev_tie = ev->tie_rtol;
  h->ev_lam_max = ev->lam_max;
  h->ev_index = index;
  double f1 = 0.0;
  int64_t na = 0;
  h->ev_on = true;
  int rc;
  if (h->n_active == 0) {
    // nothing is active: the unloaded terminal event without a solve
    // (lam = +inf from the scan, F₁ = 0; U₁ stays what the last solve left)
    if (st) std::memset(st, 0, sizeof(*st));
    h->spec_launched = false;
    rc = post_impl(h, ev->max_strain, &f1, &na, nullptr);
    if (rc) {
      drop_kept(h);
      (void)sync_stream(h);
    }
    f1 = 0.0;
  } else {
    rc = step_impl(h, dy_top, dy_bot, opts, ev->max_strain, &f1, &na, st);
  }
  h->ev_on = false;
  if (rc) return rc;
  unsigned nfail = 0;
  std::memcpy(&nfail, &h->h_red[2], sizeof nfail);
  out->lam = h->h_red[4];
  out->force1 = f1;
  out->n_failed = (int64_t)nfail;
  out->n_active = na;
  return 0;
}

int mfea_event(mfea_handle* h, double dy_top, double dy_bot, const mfea_solve_opts* opts,
               const mfea_event_opts* evopts, mfea_event_out* out, mfea_stats* st) {
  RC(event_check(evopts));  // (first: the options are checked whatever the handle)
  if (!h || !out) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_event: one partition per handle");
  if (h->bc.loads.set && h->bc.load_mode == MFEA_LOAD_DEAD) return fail(MFEA_ESTATE, kDeadLoadEvents);
  return event_impl(h, dy_top, dy_bot, opts, evopts, 0, out, st);
}

int mfea_get_displacement(mfea_handle* h, double* U) {
  if (!h || !U) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  const bool dm = partitioned(h);
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Pattern& P = pt.P;
    const int64_t N = P.n_nodes;
    std::vector<double> xp(3 * N);
    if (N) HIPC(hmemcpy(h, xp.data(), pt.x.ptr, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < N; ++i) {
      const int64_t ln = P.perm[i];
      if (dm && pt.plan.ghost[ln]) continue;
      const int64_t g = dm ? pt.plan.node_g[ln] : ln;
      for (int a = 0; a < 3; ++a) U[3 * g + a] = xp[3 * i + a];
    }
  }
  return 0;
}

int mfea_get_stress(mfea_handle* h, double* stress) {
  if (!h || !stress) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int64_t E = pt.P.n_elems;
    if (!E) continue;
    if (!partitioned(h)) {
      HIPC(hmemcpy(h, stress, pt.stress.ptr, E * sizeof(double), hipMemcpyDeviceToHost));
      continue;
    }
    std::vector<double> sl(E);
    HIPC(hmemcpy(h, sl.data(), pt.stress.ptr, E * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t le = 0; le < E; ++le)
      if (pt.plan.elem_own[le]) stress[pt.plan.elem_g[le]] = sl[le];
  }
  return 0;
}

int mfea_get_active(mfea_handle* h, uint8_t* active) {
  if (!h || !active) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const int64_t E = pt.P.n_elems;
    if (!E) continue;
    if (!partitioned(h)) {
      HIPC(hmemcpy(h, active, pt.active.ptr, E, hipMemcpyDeviceToHost));
      continue;
    }
    std::vector<uint8_t> al(E);
    HIPC(hmemcpy(h, al.data(), pt.active.ptr, E, hipMemcpyDeviceToHost));
    for (int64_t le = 0; le < E; ++le)
      if (pt.plan.elem_own[le]) active[pt.plan.elem_g[le]] = al[le];
  }
  return 0;
}

// ---------------------------------------------------------------------------
// mfea_run: the step loop with the records gathered on the device (run.hpp).
//
//   handle stream  step k | gather k → slab k&1 | step k+1 | gather k+1 | ...
//                              ↓ run_ready[k&1]        ↑ run_free[k&1] (before gather k+2)
//   copy stream            D2H slab k&1 → row k  ----→
//
// The gather reads x / stress / active on the handle's stream, behind the
// step's post (and the undo of a speculative one), so the rows are what the
// getters would return; the copy stream only ever reads the slabs.
// ---------------------------------------------------------------------------
namespace {

// the caller's record arrays, page-locked for the call
struct RunRegistered {
  void* ptr[3] = {};
  int n = 0;
  void release() {
    for (int i = 0; i < n; ++i) (void)hipHostUnregister(ptr[i]);
    n = 0;
  }
  ~RunRegistered() { release(); }
};

struct RunCtx {
  RecordSlab L;
  bool direct = true;
  uint8_t* dst[3] = {};  // U, stress, active rows of the caller (NULL = not kept)
  size_t row_b[3] = {};  // bytes per row
  int64_t off[3] = {};   // offsets in a slab
  int32_t pending = -1;  // pinned path: the row whose D2H is issued and not yet copied to dst
};

// the copy stream, events, iperm and the staging slabs of this build
int run_prepare(mfea_handle* h, Part& pt, const RecordSlab& L) {
  if (!h->run_copy) HIPC(hipStreamCreateWithFlags(&h->run_copy, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    if (!h->run_ready[i]) HIPC(hipEventCreateWithFlags(&h->run_ready[i], hipEventDisableTiming));
    if (!h->run_free[i]) HIPC(hipEventCreateWithFlags(&h->run_free[i], hipEventDisableTiming));
  }
  if (pt.rec_ok) return 0;
  const int64_t N = pt.P.n_nodes;
  if ((int64_t)pt.P.iperm.size() != N) return fail(MFEA_EINVAL, "internal: iperm does not cover the nodes");
  for (int64_t g = 0; g < N; ++g)
    if (pt.P.iperm[g] < 0 || pt.P.iperm[g] >= N) return fail(MFEA_EINVAL, "internal: iperm entry out of range");
  HIPC(pt.iperm_d.alloc(N));
  if (N) HIPC(hmemcpy(h, pt.iperm_d.ptr, pt.P.iperm.data(), N * sizeof(int32_t), hipMemcpyHostToDevice));
  for (auto& sl : pt.rec_slab) HIPC(sl.alloc((size_t)L.bytes));
  pt.rec_ok = true;
  return 0;
}

int run_pinned(mfea_handle* h, size_t bytes) {
  if (h->run_pin[0] && h->run_pin[1] && h->run_pin_bytes >= bytes) return 0;
  for (auto& p : h->run_pin) {
    if (p) (void)hipHostFree(p);
    p = nullptr;
  }
  h->run_pin_bytes = 0;
  for (auto& p : h->run_pin) HIPC(hipHostMalloc((void**)&p, std::max<size_t>(bytes, 1), hipHostMallocDefault));
  h->run_pin_bytes = bytes;
  return 0;
}

// pinned path: row k's copy has been issued; wait for it and move it to the caller's row
int run_drain(mfea_handle* h, RunCtx& c) {
  if (c.pending < 0) return 0;
  const int32_t k = c.pending;
  c.pending = -1;
  HIPC(hipEventSynchronize(h->run_free[k & 1]));
  for (int j = 0; j < 3; ++j)
    if (c.dst[j] && c.row_b[j])
      std::memcpy(c.dst[j] + (size_t)k * c.row_b[j], h->run_pin[k & 1] + c.off[j], c.row_b[j]);
  return 0;
}

// row k: the gather into slab k&1 on the handle's stream and its copy out on
// the copy stream.  lam (device memory): the rows of an event, U scaled by it
// (mfea_run_events); NULL: a step's rows
int run_emit(mfea_handle* h, Part& pt, RunCtx& c, int32_t k, const double* lam) {
  const int64_t N = pt.P.n_nodes, E = pt.P.n_elems;
  const int s = k & 1;
  uint8_t* slab = pt.rec_slab[s].ptr;
  double* u_row = c.dst[0] ? reinterpret_cast<double*>(slab + c.off[0]) : nullptr;
  double* s_row = c.dst[1] ? reinterpret_cast<double*>(slab + c.off[1]) : nullptr;
  uint8_t* a_row = c.dst[2] ? slab + c.off[2] : nullptr;
  // slab s was last read by the copies of step k - 2
  if (k >= 2) HIPC(hipStreamWaitEvent(h->stream, h->run_free[s], 0));
  if (lam)
    launch_record_event(h->stream, N, pt.iperm_d.ptr, pt.x.ptr, lam, u_row, E, pt.stress.ptr, s_row, pt.active.ptr,
                        a_row);
  else
    launch_record_step(h->stream, N, pt.iperm_d.ptr, pt.x.ptr, u_row, E, pt.stress.ptr, s_row, pt.active.ptr,
                       a_row);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(h->run_ready[s], h->stream));
  HIPC(hipStreamWaitEvent(h->run_copy, h->run_ready[s], 0));
  for (int j = 0; j < 3; ++j) {
    if (!c.dst[j] || !c.row_b[j]) continue;
    uint8_t* to = c.direct ? c.dst[j] + (size_t)k * c.row_b[j] : h->run_pin[s] + c.off[j];
    HIPC(hipMemcpyAsync(to, slab + c.off[j], c.row_b[j], hipMemcpyDeviceToHost, h->run_copy));
  }
  HIPC(hipEventRecord(h->run_free[s], h->run_copy));
  if (!c.direct) {
    // row k - 1 was copied out while step k ran: move it now, while row k's
    // copy runs, before step k + 1's copy reuses its pinned slab
    RC(run_drain(h, c));
    c.pending = k;
  }
  return 0;
}

// the record arrays of a run of n_rows rows: slab layout, staging, page-locking
// (or the pinned slabs where that fails)
int run_open(mfea_handle* h, Part& pt, RunCtx& c, RunRegistered& reg, int32_t n_rows, double* U, double* stress,
             uint8_t* active) {
  c.L = record_slab(pt.P.n_nodes, pt.P.n_elems);
  RC(run_prepare(h, pt, c.L));
  c.dst[0] = reinterpret_cast<uint8_t*>(U);
  c.dst[1] = reinterpret_cast<uint8_t*>(stress);
  c.dst[2] = active;
  c.row_b[0] = (size_t)pt.P.n_nodes * 24;
  c.row_b[1] = (size_t)pt.P.n_elems * 8;
  c.row_b[2] = (size_t)pt.P.n_elems;
  c.off[0] = c.L.off_u;
  c.off[1] = c.L.off_s;
  c.off[2] = c.L.off_a;
  c.direct = h->opt_run_register;
  for (int j = 0; j < 3 && c.direct; ++j) {
    if (!c.dst[j] || !c.row_b[j]) continue;
    if (hipHostRegister(c.dst[j], (size_t)n_rows * c.row_b[j], hipHostRegisterDefault) == hipSuccess) {
      reg.ptr[reg.n++] = c.dst[j];
    } else {
      (void)hipGetLastError();
      c.direct = false;
    }
  }
  if (!c.direct) {
    reg.release();
    RC(run_pinned(h, (size_t)c.L.bytes));
  }
  h->run_direct = c.direct ? 1 : 0;
  return 0;
}

// every exit of a run: the copies issued so far land before the arrays are released
int run_close(mfea_handle* h, RunCtx& c, RunRegistered& reg, int rc, const char* who) {
  const int rd = run_drain(h, c);
  const hipError_t es = hipStreamSynchronize(h->run_copy);
  reg.release();
  if (rc == 0) rc = rd;
  if (rc == 0 && es != hipSuccess)
    rc = fail(MFEA_EDEVICE, std::string(who) + ": copy stream: " + hipGetErrorString(es));
  return rc;
}

int run_steps(mfea_handle* h, Part& pt, RunCtx& c, int32_t n_steps, const double* dy_top, const double* dy_bot,
              const mfea_solve_opts* opts, double max_strain, const mfea_run_records* rec, int32_t* n_done,
              int32_t* stop_reason) {
  for (int32_t k = 0; k < n_steps; ++k) {
    double force = 0.0;
    int64_t na = 0;
    mfea_stats st;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = mfea_step(h, dy_top[k], dy_bot[k], opts, max_strain, &force, &na, &st);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc == MFEA_EMAXIT || rc == MFEA_EBREAKDOWN) {
      *stop_reason = rc;
      return 0;
    }
    if (rc) return rc;
    rec->force[k] = force;
    rec->n_active[k] = na;
    if (rec->stats) rec->stats[k] = st;
    if (rec->wall_s) rec->wall_s[k] = wall;
    RC(run_emit(h, pt, c, k, nullptr));
    *n_done = k + 1;
    if (na == 0) {
      *stop_reason = MFEA_RUN_NO_ACTIVE;
      return 0;
    }
  }
  return 0;
}

}  // namespace

int mfea_run(mfea_handle* h, int32_t n_steps, const double* dy_top, const double* dy_bot,
             const mfea_solve_opts* opts, double max_strain, const mfea_run_records* rec, int32_t* n_done,
             int32_t* stop_reason) {
  if (!h || !rec || !n_done || !stop_reason) return fail(MFEA_EINVAL, "NULL argument");
  if (n_steps < 0) return fail(MFEA_EINVAL, "negative n_steps");
  if (n_steps && (!dy_top || !dy_bot || !rec->force || !rec->n_active))
    return fail(MFEA_EINVAL, "mfea_run: dy_top, dy_bot, force and n_active are required");
  *n_done = 0;
  *stop_reason = MFEA_RUN_COMPLETE;
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h))
    return fail(MFEA_ESTATE, "mfea_run: one partition per handle (the records of a partitioned handle "
                             "need its ownership maps on the device)");
  if (n_steps == 0) return 0;
  Part& pt = part0(h);
  RunCtx c;
  RunRegistered reg;
  RC(run_open(h, pt, c, reg, n_steps, rec->U, rec->stress, rec->active));
  const int rc = run_steps(h, pt, c, n_steps, dy_top, dy_bot, opts, max_strain, rec, n_done, stop_reason);
  return run_close(h, c, reg, rc, "mfea_run");
}

// The event loop of mfea_run_events: n_events × mfea_event, each followed by
// its record rows (the U row scaled by the event's lam on the device).
int mfea_run_events(mfea_handle* h, int32_t n_events, double dy_top, double dy_bot, const mfea_solve_opts* opts,
                    const mfea_event_opts* evopts, const mfea_event_records* rec, int32_t* n_done,
                    int32_t* stop_reason) {
  RC(event_check(evopts));
  if (!h || !rec || !n_done || !stop_reason) return fail(MFEA_EINVAL, "NULL argument");
  if (n_events < 0) return fail(MFEA_EINVAL, "negative n_events");
  if (n_events && (!rec->lam || !rec->force1 || !rec->n_failed || !rec->n_active))
    return fail(MFEA_EINVAL, "mfea_run_events: lam, force1, n_failed and n_active are required");
  *n_done = 0;
  *stop_reason = MFEA_EVENTS_COMPLETE;
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_run_events: one partition per handle");
  if (h->bc.loads.set && h->bc.load_mode == MFEA_LOAD_DEAD) return fail(MFEA_ESTATE, kDeadLoadEvents);
  Part& pt = part0(h);
  const int64_t E = pt.P.n_elems;
  if (E) HIPC(hipMemsetAsync(pt.event_of.ptr, 0xFF, E * sizeof(int32_t), h->stream));
  int rc = 0;
  if (n_events > 0) {
    RunCtx c;
    RunRegistered reg;
    RC(run_open(h, pt, c, reg, n_events, rec->U, rec->stress, rec->active));
    for (int32_t k = 0; k < n_events && rc == 0; ++k) {
      mfea_event_out out;
      mfea_stats st;
      const auto t0 = std::chrono::steady_clock::now();
      rc = event_impl(h, dy_top, dy_bot, opts, evopts, k, &out, &st);
      const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (rc == MFEA_EMAXIT || rc == MFEA_EBREAKDOWN) {
        *stop_reason = rc;
        rc = 0;
        break;
      }
      if (rc) break;
      rec->lam[k] = out.lam;
      rec->force1[k] = out.force1;
      rec->n_failed[k] = out.n_failed;
      rec->n_active[k] = out.n_active;
      if (rec->stats) rec->stats[k] = st;
      if (rec->wall_s) rec->wall_s[k] = wall;
      rc = run_emit(h, pt, c, k, pt.red.ptr + 8);
      if (rc) break;
      *n_done = k + 1;
      if (out.n_failed == 0) {  // terminal: smax = 0 (unloaded) or lam > lam_max
        // (with a per-element strength h_red[3] is the scan's lam: +inf when unloaded)
        const bool loaded = h->pe_S.empty() ? h->h_red[3] > 0.0 : std::isfinite(h->h_red[3]);
        *stop_reason = loaded ? MFEA_EVENTS_LAMBDA_MAX : MFEA_EVENTS_UNLOADED;
        break;
      }
    }
    rc = run_close(h, c, reg, rc, "mfea_run_events");
  }
  if (rc == 0 && rec->event_of && E)
    HIPC(hmemcpy(h, rec->event_of, pt.event_of.ptr, E * sizeof(int32_t), hipMemcpyDeviceToHost));
  return rc;
}

int mfea_element_stiffness(mfea_handle* h, int64_t n, const double* p1s, const double* p2s,
                           double E, double A, double I, double* Ke, double* L) {
  if (!h || n < 0 || (n && (!p1s || !p2s || !Ke || !L))) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  if (n == 0) return 0;
  Material m;
  m.EA = E * A;
  m.EI12 = (12.0 * E) * I;
  m.E = E;
  DevBuf<double> a, b, k, l;
  HIPC(a.alloc(3 * n));
  HIPC(b.alloc(3 * n));
  HIPC(k.alloc(36 * n));
  HIPC(l.alloc(n));
  HIPC(hipMemcpyAsync(a.ptr, p1s, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(b.ptr, p2s, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_element_stiffness(h->stream, n, a.ptr, b.ptr, m, k.ptr, l.ptr);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(Ke, k.ptr, 36 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipMemcpyAsync(L, l.ptr, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return 0;
}

int mfea_export_csr(mfea_handle* h, int64_t* nnz, int64_t* indptr, int32_t* indices,
                    double* data) {
  if (!h || !nnz) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_export_csr: single-partition handles only");
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  const int64_t N = P.n_nodes, E = P.n_elems;
  std::vector<double> diag6(6 * N), val6(6 * pt.G);
  std::vector<uint8_t> act(E);
  if (N) HIPC(hmemcpy(h, diag6.data(), pt.diag.ptr, 6 * N * sizeof(double), hipMemcpyDeviceToHost));
  if (pt.G) HIPC(hmemcpy(h, val6.data(), pt.val.ptr, 6 * pt.G * sizeof(double), hipMemcpyDeviceToHost));
  if (E) HIPC(hmemcpy(h, act.data(), pt.active.ptr, E, hipMemcpyDeviceToHost));
  std::vector<int64_t> ip;
  std::vector<int32_t> ix;
  std::vector<double> dv;
  export_csr(P, act, diag6, val6, ip, ix, dv);
  if (!indptr) {
    *nnz = (int64_t)ix.size();
    return 0;
  }
  if (*nnz < (int64_t)ix.size()) return fail(MFEA_EINVAL, "output arrays too small");
  *nnz = (int64_t)ix.size();
  std::memcpy(indptr, ip.data(), ip.size() * sizeof(int64_t));
  std::memcpy(indices, ix.data(), ix.size() * sizeof(int32_t));
  std::memcpy(data, dv.data(), dv.size() * sizeof(double));
  return 0;
}

int mfea_solve_csr(mfea_handle* h, int64_t n, const int64_t* indptr, const int32_t* indices,
                   const double* data, int64_t n_known, const int64_t* known_dofs,
                   const double* known_vals, const mfea_solve_opts* opts, double* U,
                   mfea_stats* st) {
  if (!h || n < 0 || (n && (!indptr || !U)) || n_known < 0 || (n_known && (!known_dofs || !known_vals)))
    return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  if (h->world > 1) return fail(MFEA_ESTATE, "mfea_solve_csr: not on a partitioned (RCCL) handle");
  mfea_solve_opts o = opts ? *opts : default_opts();
  if (o.precond != MFEA_PC_JACOBI) return fail(MFEA_EINVAL, "CSR path supports Jacobi only");
  if (st) std::memset(st, 0, sizeof(*st));
  if (n == 0) return 0;
  const int64_t nnz = indptr[n];
  for (int64_t t = 0; t < nnz; ++t)
    if (indices[t] < 0 || indices[t] >= n) return fail(MFEA_EINVAL, "column index out of range");
  std::vector<uint8_t> known(n, 0);
  std::vector<double> kval(n, 0.0);
  for (int64_t i = 0; i < n_known; ++i) {
    const int64_t k = known_dofs[i];
    if (k < 0 || k >= n) return fail(MFEA_EINVAL, "known dof out of range");
    known[k] = 1;
    kval[k] = known_vals[i];
  }
  hipStream_t s = h->stream;
  Part& pt = part0(h);  // its reduction scratch, slots and state
  HIPC(h->c_indptr.alloc(n + 1));
  HIPC(h->c_indices.alloc(nnz));
  HIPC(h->c_data.alloc(nnz));
  HIPC(h->c_known.alloc(n));
  HIPC(h->c_kval.alloc(n));
  HIPC(h->c_x.alloc(n));
  HIPC(h->c_r.alloc(n));
  HIPC(h->c_p.alloc(n));
  HIPC(h->c_q.alloc(n));
  HIPC(h->c_dinv.alloc(n));
  const int64_t maxg = std::max<int64_t>(grid_rows(n), 2048);
  if (pt.partials.n < (size_t)(4 * maxg)) HIPC(pt.partials.alloc(4 * (maxg + 16)));
  if (!pt.red.ptr) {
    HIPC(pt.red.alloc(16));
    HIPC(hipMemsetAsync(pt.red.ptr, 0, 16 * sizeof(double), s));
  }
  if (!pt.tickets.ptr) {
    HIPC(pt.tickets.alloc(kTicketSets * kTicketStride));
    HIPC(hipMemsetAsync(pt.tickets.ptr, 0, kTicketSets * kTicketStride * sizeof(unsigned), s));
  }
  HIPC(pt.slots.alloc(kMaxChunk + 2));
  HIPC(pt.state.alloc(1));
  HIPC(hipMemcpyAsync(h->c_indptr.ptr, indptr, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (nnz) {
    HIPC(hipMemcpyAsync(h->c_indices.ptr, indices, nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(h->c_data.ptr, data, nnz * sizeof(double), hipMemcpyHostToDevice, s));
  }
  HIPC(hipMemcpyAsync(h->c_known.ptr, known.data(), n, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(h->c_kval.ptr, kval.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(h->c_q.ptr, 0, n * sizeof(double), s));
  HIPC(hipEventRecord(h->ev[1], s));
  launch_csr_rhs_init(s, n, h->c_indptr.ptr, h->c_indices.ptr, h->c_data.ptr, h->c_known.ptr,
                      h->c_kval.ptr, o.reg, h->c_x.ptr, h->c_r.ptr, h->c_p.ptr, h->c_dinv.ptr,
                      pt.partials.ptr, tix(pt, 5), pt.red.ptr);
  launch_init_finalize(s, pt.red.ptr, o.rtol, o.atol, o.norm, o.max_it, o.reg, pt.slots.ptr,
                       pt.state.ptr);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(h->ev[2], s));
  const int chunk = o.chunk > 0 ? std::min(o.chunk, kMaxChunk) : 32;
  SolveState fin;
  int rc = drive_chunks(
      h, chunk, o.max_it,
      [&]() -> int {
        for (int j = 0; j < chunk; ++j) {
          launch_spmv_csr(s, j, n, h->c_indptr.ptr, h->c_indices.ptr, h->c_data.ptr,
                          h->c_known.ptr, o.reg, h->c_p.ptr, h->c_q.ptr, pt.slots.ptr,
                          pt.state.ptr, pt.partials.ptr, tix(pt, 6));
          launch_update(s, j, n, 0, h->c_x.ptr, h->c_r.ptr, h->c_p.ptr, h->c_q.ptr, h->c_dinv.ptr,
                        pt.slots.ptr, pt.state.ptr, pt.partials.ptr, tix(pt, 7));
          launch_direction(s, j, n, 0, h->c_r.ptr, h->c_p.ptr, h->c_dinv.ptr, pt.slots.ptr,
                           pt.state.ptr);
        }
        launch_advance(s, chunk, pt.slots.ptr, pt.state.ptr);
        HIPC(hipGetLastError());
        return 0;
      },
      &fin);
  if (rc) return rc;
  HIPC(hipEventRecord(h->ev[3], s));
  HIPC(hipMemcpyAsync(U, h->c_x.ptr, n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  if (st) {
    st->iters = fin.iters;
    st->status = fin.status;
    st->bnorm = std::sqrt(fin.bb0);
    st->relres = fin.res0 > 0 ? std::sqrt(fin.res_final / fin.res0) : 0.0;
    st->n_free = n - (int64_t)std::count(known.begin(), known.end(), 1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[2], h->ev[3]);
    st->t_solve_ms = ms;
  }
  if (fin.status == -4) return fail(MFEA_EMAXIT, "PCG reached max_it without converging");
  if (fin.status == -5) return fail(MFEA_EBREAKDOWN, "PCG breakdown");
  return 0;
}

int mfea_get_info(mfea_handle* h, mfea_info* info) {
  if (!h || !info) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  std::memset(info, 0, sizeof(*info));
  info->n_nodes = P.n_nodes;
  info->n_elems = P.n_elems;
  info->n_free_nodes = P.n_free;
  info->n_top = P.n_top;
  info->n_known = P.n_known;
  info->n_slices = P.n_slices();
  info->n_slots = pt.G;
  int64_t inc = 0;
  for (int64_t i = 0; i < P.n_free; ++i) inc += P.row_len[i];
  info->free_incidences = inc;
  info->planar = h->planar ? 1 : 0;
  info->cg_lanes = use_ell(h, pt) ? 1 : 0;
  info->n_lanes = pt.ell_ok ? pt.L.n_lanes : 0;
  int64_t halo = 0;
  if (pt.ell_ok)
    for (int32_t p : pt.L.partner) halo += p != -1;
  info->n_halo = halo;
  info->n_parts = nranks(h);
  info->part = pt.rank;
  info->n_pairs = pt.plan.n_pairs;
  info->n_ghost = P.n_ghost;
  if (pt.ell_ok) {
    info->halo_compact = pt.ell_hc ? 1 : 0;
    info->block_size = ell_block_size(ell_op(h, pt));
    info->grid = ell_grid_size(ell_op(h, pt));
  }
  return 0;
}

// iteration 0 of the active CG kernel of partition 0 (profiling / tracing;
// partitioned handles: the per-GPU kernel without its exchange)
static void launch_iter0(mfea_handle* h, int pc, unsigned long long* trace) {
  Part& pt = part0(h);
  if (use_ell(h, pt))
    launch_ell_iter(h->stream, 0, ell_op(h, pt), pc, ell_vecs(pt), pt.slots.ptr, pt.state.ptr,
                    pt.cg_part.ptr, trace);
  else
    launch_cg_iter(h->stream, 0, sell_op(pt), pc, cg_vecs(pt), pt.slots.ptr, pt.state.ptr,
                   pt.cg_part.ptr, trace);
}

int mfea_profile_spmv(mfea_handle* h, int reps, double* avg_ms) {
  if (!h || !avg_ms || reps <= 0) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  RC(ensure_built(h));
  // partitioned: partition 0's w kernel over its own rows (the plan its device
  // arrays hold: its block-Jacobi hierarchy or its share of the global one)
  Part& pt = part0(h);
  drop_kept(h);  // (conservative: the profile launches run on the solve's arrays)
  if (!(partitioned(h) ? pt.dev_plan >= 0 : pt.amg_ok)) return fail(MFEA_ESTATE, "profile the SpMV after a GAMG solve");
  hipStream_t s = h->stream;
  const int nd = pt.dev_plan == 1 ? h->gamg.nd : pt.amg.nd;
  hipGraph_t g;
  hipGraphExec_t ge = nullptr;
  HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  for (int k = 0; k < reps; ++k) launch_amg_cg_w(s, nd, 0, true, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr);
  HIPC(hipStreamEndCapture(s, &g));
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  HIPC(e);
  e = hipGraphLaunch(ge, s);  // warm
  if (e == hipSuccess) e = hipEventRecord(h->ev[0], s);
  if (e == hipSuccess) e = hipGraphLaunch(ge, s);
  if (e == hipSuccess) e = hipEventRecord(h->ev[1], s);
  if (e == hipSuccess) e = hipEventSynchronize(h->ev[1]);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
  (void)hipGraphExecDestroy(ge);
  HIPC(e);
  *avg_ms = ms / reps;
  return 0;
}

int mfea_profile_iteration(mfea_handle* h, int precond, int reps, double* avg_ms) {
  if (!h || !avg_ms || reps <= 0) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  RC(ensure_built(h));
  Part& pt = part0(h);
  hipStream_t s = h->stream;
  drop_kept(h);  // (conservative: the profile launches run on the solve's arrays)
  if (precond == MFEA_PC_GAMG || precond == MFEA_PC_SOR || precond == MFEA_PC_ICC) {
    if (!pt.amg_ok || pt.amg_kind != precond)
      return fail(MFEA_ESTATE, "profile GAMG / SOR / ICC after a solve with that preconditioner");
    // Running state: slots[0] = INIT and real partials from an ungated first
    // w kernel; every rep is update + V-cycle + w(first) — the full work of
    // one PCG iteration, all stores included.
    const int nd = pt.amg.nd;
    launch_amg_cg_w(s, nd, 0, true, pt.amg_lev[0], pt.amg_cg, pt.slots.ptr, pt.cg_part.ptr);
    launch_cg_init_finalize(s, pt.red.ptr + 8, 0.0, 0.0, 0, 1 << 30, 1e-12, pt.state.ptr);
    // the reps iterations replay as one captured graph, as in the solve
    // (eager launches of ≈ 20 short kernels per iteration are host-bound)
    hipGraph_t g;
    hipGraphExec_t ge = nullptr;
    HIPC(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    for (int k = 0; k < reps; ++k) enqueue_amg_iteration(h, pt, 0, true);
    HIPC(hipStreamEndCapture(s, &g));
    hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPC(e);
    e = hipGraphLaunch(ge, s);  // warm
    if (e == hipSuccess) e = hipEventRecord(h->ev[0], s);
    if (e == hipSuccess) e = hipGraphLaunch(ge, s);
    if (e == hipSuccess) e = hipEventRecord(h->ev[1], s);
    if (e == hipSuccess) e = hipEventSynchronize(h->ev[1]);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
    (void)hipGraphExecDestroy(ge);
    HIPC(e);
    *avg_ms = ms / reps;
    return 0;
  }
  const int pc = precond == MFEA_PC_BLOCK_JACOBI ? 1 : 0;
  // Running state with tol 0: slots[0] = INIT and parity-0 partials of 1, so
  // γ = δ = ‖r‖² = ‖u‖² = G > 0, α = 1, β = 0.  Every launch is iteration 0
  // (same parity), so it reads the same buffers and does identical work
  // (including all stores); only x and p drift.
  const double ones[2] = {1.0, 1.0};
  HIPC(hipMemcpyAsync(pt.red.ptr + 8, ones, sizeof(ones), hipMemcpyHostToDevice, s));
  launch_cg_init_finalize(s, pt.red.ptr + 8, 0.0, 0.0, 0, 1 << 30, 1e-12, pt.state.ptr);
  std::vector<double> pones(4 * kCgMaxPartials, 1.0);
  HIPC(hipMemcpyAsync(pt.cg_part.ptr, pones.data(), pones.size() * sizeof(double),
                      hipMemcpyHostToDevice, s));
  Slot s0;
  std::memset(&s0, 0, sizeof(s0));
  s0.flag = kInit;
  HIPC(hipMemcpyAsync(pt.slots.ptr, &s0, sizeof(s0), hipMemcpyHostToDevice, s));
  launch_iter0(h, pc, nullptr);  // warm
  HIPC(hipEventRecord(h->ev[0], s));
  for (int k = 0; k < reps; ++k) launch_iter0(h, pc, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(h->ev[1], s));
  HIPC(hipEventSynchronize(h->ev[1]));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
  *avg_ms = ms / reps;
  return 0;
}

int mfea_debug_trace_iteration(mfea_handle* h, int precond, uint64_t* out, int64_t cap,
                               int64_t* n_waves) {
  if (!h || !out || !n_waves || cap < 0) return fail(MFEA_EINVAL, "bad argument");
  double ms = 0;
  RC(mfea_profile_iteration(h, precond, 20, &ms));  // same running state
  hipStream_t s = h->stream;
  Part& pt = part0(h);
  const bool ell = use_ell(h, pt);
  const int64_t g = ell ? ell_grid_size(ell_op(h, pt)) : cg_grid(pt.P.n_free);
  const int64_t nw = g * ((ell ? ell_block_size(ell_op(h, pt)) : cg_block_size(0)) / 64);
  if (cap < nw * 4) return fail(MFEA_EINVAL, "trace buffer too small");
  unsigned long long* d = nullptr;
  HIPC(hipMalloc(&d, nw * 4 * sizeof(unsigned long long)));
  HIPC(hipMemsetAsync(d, 0, nw * 4 * sizeof(unsigned long long), s));
  launch_iter0(h, precond == MFEA_PC_BLOCK_JACOBI ? 1 : 0, d);
  hipError_t e = hipMemcpyAsync(out, d, nw * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(MFEA_EDEVICE, hipGetErrorString(e));
  *n_waves = nw;
  return 0;
}

int mfea_debug_amg_info(mfea_handle* h, int* n_levels, int64_t* rows, int64_t* blocks,
                        int64_t* pblocks, int cap, int64_t* pair_items, int* nd, int* n_dist,
                        int64_t* ptblocks) {
  if (!h || !n_levels || cap < 0 || (cap && (!rows || !blocks || !pblocks)))
    return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  RC(ensure_built(h));
  bool rebuilt = false;
  if (partitioned(h) && !h->opt_amg_dist) return fail(MFEA_ESTATE, "GAMG block Jacobi: per-partition hierarchies");
  if (partitioned(h)) RC(ensure_gamg(h, &rebuilt));
  else RC(ensure_amg(h, part0(h), &rebuilt));
  const AmgPlan& pl = partitioned(h) ? h->gamg : part0(h).amg;
  if (n_dist) *n_dist = pl.n_dist;
  *n_levels = (int)pl.lev.size();
  for (int l = 0; l < std::min(cap, *n_levels); ++l) {
    const SellPat& A = pl.lev[l].A;
    rows[l] = A.n;
    int64_t nb = 0;
    for (int64_t i = 0; i < A.n; ++i) nb += A.rlen[i];
    blocks[l] = nb;
    int64_t pb = 0;
    for (int32_t r : pl.lev[l].P.rlen) pb += r;
    pblocks[l] = pb;
    if (ptblocks) {
      int64_t tb = 0;
      for (int32_t r : pl.lev[l].PT.rlen) tb += r;
      ptblocks[l] = tb;
    }
  }
  if (pair_items) *pair_items = pl.pair_items;
  if (nd) *nd = pl.nd;
  return 0;
}

static_assert(kOptSweepPieceMax == kSweepPieceLen && kOptBigChunkMax == mfea_handle::kRemGraphs - 1,
              "options.hpp's bounds");

// what setting an option does beyond its field (options.hpp OptEffect)
static int option_effect(mfea_handle* h, OptEffect e) {
  switch (e) {
    case OptEffect::kNone:
      break;
    case OptEffect::kLevelLanes:
      for (auto& pp : h->parts)
        for (auto& L : pp->amg_lev) set_level_lanes(*h, L);
      break;
    case OptEffect::kCycle:
      for (auto& pp : h->parts) {
        pp->amg_cg.cycle = h->opt_amg_cycle;
        for (auto& L : pp->amg_lev)
          if (L.PT.n > 0) L.compact = h->opt_amg_cycle;
        if (!pp->amg_lev.empty() && pp->amg_levd.n >= pp->amg_lev.size())
          HIPC(hmemcpy(h, pp->amg_levd.ptr, pp->amg_lev.data(), pp->amg_lev.size() * sizeof(AmgLevD),
                       hipMemcpyHostToDevice));
      }
      break;
    case OptEffect::kOmega: h->amg_safe_omega = false; break;
    case OptEffect::kReuse:  // the next solve builds for its own set
      for (auto& pp : h->parts) pp->amg_stale = true;
      break;
    case OptEffect::kDistAuto: h->amg_auto.gen = -1; break;
    case OptEffect::kGlobalPlan: h->gamg_ok = false; break;
    case OptEffect::kDistSums:
      for (auto& pp : h->parts) pp->amg_dist.zero_w = h->opt_dist_sums && h->world > 1 ? h->world : 0;
      break;
  }
  return 0;
}

static int option_error(const OptionDesc& d) {
  return fail(MFEA_EINVAL, std::string(d.name) + ": " + d.legal_text);
}

int mfea_set_option(mfea_handle* h, const char* name, int64_t value) {
  if (!h || !name) return fail(MFEA_EINVAL, "NULL argument");
  const OptionDesc* d = find_option(name);
  if (!d) return fail(MFEA_EINVAL, std::string("unknown option ") + name);
  if (!option_legal(*d, value)) return option_error(*d);
  option_store(*d, *h, value);
  RC(option_effect(h, d->effect));
  // kept K / hierarchy values: dropped by every option but the few that
  // cannot change a value (conservative: most options only change launches)
  if (!option_keeps(*d, value)) drop_kept(h);
  destroy_graph(h);  // captured graphs hold the old geometry (dist_sums: the old exchange)
  if (d->rebuilds_layout) {
    if (!h->dirty && h->Ecount) {  // keep the current activity across the rebuild
      RC(set_device(h));
      RC(gather_active(h, h->active_host));
    }
    h->dirty = true;
  }
  return 0;
}

int mfea_debug_option_check(const char* name, int64_t value, int64_t* stored) {
  if (!name || !stored) return fail(MFEA_EINVAL, "NULL argument");
  const OptionDesc* d = find_option(name);
  if (!d) return fail(MFEA_EINVAL, std::string("unknown option ") + name);
  if (!option_legal(*d, value)) return option_error(*d);
  Options scratch;
  option_store(*d, scratch, value);
  *stored = d->load(scratch);
  return 0;
}

int mfea_debug_amg_vcycle(mfea_handle* h, const double* r, double* u) {
  if (!h || !r || !u) return fail(MFEA_EINVAL, "NULL argument");
  RC(set_device(h));
  RC(ensure_built(h));
  hipStream_t s = h->stream;
  const bool dm = partitioned(h);
  if (dm && !h->opt_amg_dist) return fail(MFEA_ESTATE, "mfea_debug_amg_vcycle: amg_dist 0 is not one operator");
  drop_kept(h);  // (the setup below re-forms the hierarchy's values at its own reg)
  bool rebuilt = false;
  if (dm) {
    RC(ensure_gamg(h, &rebuilt));
    RC(enqueue_gamg_setup(h, 1e-12));
  } else {
    RC(ensure_amg(h, part0(h), &rebuilt));
    enqueue_amg_setup(h, part0(h), 1e-12);
  }
  const int nd = dm ? h->gamg.nd : part0(h).amg.nd;
  // r (node order) → each partition's row-order RHS buffer (its q), then
  // the CG init (r, x = ω D⁻¹ r) and one V-cycle
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const Pattern& P = pt.P;
    std::vector<double> b(3 * P.n_nodes, 0.0);
    for (int64_t i = 0; i < P.n_free; ++i) {
      const int64_t g = dm ? pt.plan.node_g[P.perm[i]] : P.perm[i];
      for (int a = 0; a < nd; ++a) b[3 * i + a] = r[nd * g + a];
    }
    HIPC(hmemcpy(h, pt.q.ptr, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
    launch_amg_cg_init(s, nd, pt.amg_lev[0], pt.amg_cg, pt.q.ptr);
  }
  if (dm) {
    RC(enqueue_gamg_vcycle(h, -1));
  } else {
    Part& pt = part0(h);
    launch_amg_vcycle(s, nd, pt.amg_lev.data(), (int)pt.amg_lev.size(), pt.amg_cg, pt.amg_tail, nullptr);
  }
  HIPC(hipGetLastError());
  RC(sync_stream(h));
  std::memset(u, 0, (size_t)h->N * nd * sizeof(double));
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const AmgCg& cg = pt.amg_cg;
    std::vector<float> uf((size_t)nd * cg.n);
    std::vector<int32_t> row0(cg.n);
    if (cg.n) {
      HIPC(hmemcpy(h, uf.data(), cg.u, uf.size() * sizeof(float), hipMemcpyDeviceToHost));
      HIPC(hmemcpy(h, row0.data(), cg.row0, row0.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    for (int64_t i = cg.lo; i < cg.hi; ++i) {
      const int64_t lr = row0[i];
      const int64_t g = dm ? pt.plan.node_g[pt.P.perm[lr]] : pt.P.perm[lr];
      for (int a = 0; a < nd; ++a) u[nd * g + a] = uf[nd * i + a];
    }
  }
  return 0;
}

int mfea_debug_amg_vector(mfea_handle* h, int l, int which, double* out, int64_t cap, int64_t* n) {
  if (!h || !n || which < 0 || which > 6) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  const bool dm = partitioned(h);
  const AmgPlan& pl = dm ? h->gamg : part0(h).amg;
  if (l < 0 || l >= (int)pl.lev.size()) return fail(MFEA_EINVAL, "level out of range");
  const int nd = pl.nd;
  const AmgLevel& L = pl.lev[l];
  *n = L.A.n;
  const int w = which >= 4 && which != 5 ? nd * nd : nd;  // per-row width
  if (!out) return 0;
  // the device must hold the plan pl describes (a partitioned handle may hold
  // the block-Jacobi plans after amg_dist 0 or an automatic choice of it)
  if (dm)
    for (auto& pp : h->parts)
      if (pp->dev_plan != 1) return fail(MFEA_ESTATE, "the device holds the block-Jacobi plans: run amg_vcycle first");
  if (cap < w * L.A.n) return fail(MFEA_EINVAL, "output too small");
  for (auto& pp : h->parts) {
    Part& pt = *pp;
    const AmgLevD& d = pt.amg_lev[l];
    std::vector<double> v((size_t)w * L.A.n, 0.0);
    if (which == 4) {  // D⁻¹ blocks
      std::vector<float> f(v.size());
      HIPC(hmemcpy(h, f.data(), d.dinv32, f.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < f.size(); ++k) v[k] = f[k];
    } else if (which == 5) {  // the Gershgorin bound g, every row
      double om[2];
      HIPC(hmemcpy(h, om, d.omega, sizeof(om), hipMemcpyDeviceToHost));
      std::fill(v.begin(), v.end(), om[1]);
    } else if (which == 6) {  // diagonal blocks of A (slot 0 of every row)
      std::vector<float> a((size_t)nd * nd * d.A.npos);
      HIPC(hmemcpy(h, a.data(), d.A.val32, a.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < L.A.n; ++i)
        for (int c = 0; c < nd * nd; ++c) v[(size_t)nd * nd * i + c] = a[(size_t)nd * nd * L.A.pos(i, 0) + c];
    } else if (l == 0 && (which == 0 || which == 3)) {
      if (which == 0) {
        HIPC(hmemcpy(h, v.data(), pt.amg_cg.r, v.size() * sizeof(double), hipMemcpyDeviceToHost));
      } else {
        std::vector<float> f(v.size());
        HIPC(hmemcpy(h, f.data(), pt.amg_cg.u, f.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < f.size(); ++k) v[k] = f[k];
      }
    } else {
      const float* src = which == 0 ? d.b : which == 1 ? d.x : which == 2 ? d.t : d.e;
      if (!src) return fail(MFEA_EINVAL, "no such vector on this level");
      std::vector<float> f(v.size());
      HIPC(hmemcpy(h, f.data(), src, f.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < f.size(); ++k) v[k] = f[k];
    }
    const bool split = dm && l < pl.n_dist;
    const int64_t lo = split ? pt.amg_rank.lo[l] : 0, hi = split ? pt.amg_rank.hi[l] : L.A.n;
    if (!split && pt.rank != 0) continue;
    for (int64_t i = lo; i < hi; ++i)
      for (int a = 0; a < w; ++a) out[(size_t)w * L.nat[i] + a] = v[(size_t)w * i + a];
  }
  return 0;
}

// The read-only names of mfea_get_option: name, value, and whether it is read
// from partition 0's plan (MFEA_ESTATE before there is one; p is null there).
namespace {
int64_t stored_blocks(const std::vector<int32_t>& col) {
  int64_t nb = 0;
  for (int32_t c : col) nb += c >= 0;
  return nb;
}
int64_t asm_colours(const mfea_handle* h) {
  int64_t nc = 0;
  for (auto& pp : h->parts) nc = std::max<int64_t>(nc, pp->ec_state > 0 ? pp->ec.colors : 0);
  return nc;
}
struct ReadOnly {
  const char* name;
  bool part;
  int64_t (*get)(const mfea_handle* h, const Part* p);
};
#define RO(name, part, expr) \
  {name, part, [](const mfea_handle* h, const Part* p) -> int64_t { return (void)h, (void)p, expr; }}
const ReadOnly kReadOnly[] = {
    RO("element_props", false, h->has_props()),  // per-element columns are set
    RO("run_direct", false, h->run_direct),      // the last mfea_run's host path
    RO("amg_merged", true, p->amg_mg.on),        // the plan's cycle form
    RO("amg_merge_dq_blocks", true, p->amg_mplan.on ? stored_blocks(p->amg_mplan.DQ.col) : 0),
    RO("amg_merge_u_blocks", true, p->amg_mplan.on ? stored_blocks(p->amg_mplan.U.col) : 0),
    RO("sweep_colors", true, p->sweep.colors),
    RO("sweep_pieces", true, p->sweep.n_pieces),
    // partition 0's plan: the fused launch is in use; level 0's window; the
    // largest block halo and the capacity it was held against
    RO("amg_fused_l0", false, p && amg_fused(h, *p)),
    RO("amg_l0_window_used", false, p ? p->amg.l0_window : 0),
    RO("amg_fuse_max_halo", false, p ? p->amg_fplan.max_halo : 0),
    RO("amg_fuse_halo_cap", false, p ? amg_fuse_halo_cap(p->amg.nd, p->amg.l0_window) : 0),
    RO("amg_safe_omega", false, h->amg_safe_omega),
    // partition 0's collapsed level kc (0: none), the stored blocks of its V
    RO("amg_collapse_level", false, p ? p->amg_coll.kc : 0),
    RO("amg_collapse_blocks", false, p && p->amg_coll.kc > 0 ? stored_blocks(p->amg_coll.lev[0].V.col) : 0),
    RO("amg_spatial_chosen", false, p && p->amg.spatial),  // the plan is in Z-order
    RO("amg_reused", true, p->amg_reused),  // the last solve kept a hierarchy built for another set
    RO("amg_build_iters", true, p->amg_build_iters),
    // the partitioned form in use (-1: the automatic choice still undecided)
    RO("amg_dist_chosen", false, h->opt_amg_dist >= 0 ? h->opt_amg_dist : h->amg_auto.choice),
    RO("op_kept_steps", false, h->op_kept_steps),      // steps that skipped the assembly
    RO("amg_setup_kept", false, h->amg_setup_kept),    // solves that skipped the numeric setup
    RO("amg_px_replays", false, h->amg_px_replays),    // p, x replay launches the solves queued
    RO("amg_px_slots", false, kAmgPxSlots),            // u slots of the lazy p, x chain
    RO("amg_start_fused", false, h->amg_start_fused),  // solves that started with k_amg_start
    RO("amg_close_hits", false, h->amg_close_hits),    // solves ended by the closing check
    RO("amg_last_cycles", false, h->amg_last_cycles),  // V-cycles the last solve queued
    RO("asm_colours", false, asm_colours(h)),
};
#undef RO
}  // namespace

int mfea_get_option(mfea_handle* h, const char* name, int64_t* value) {
  if (!h || !name || !value) return fail(MFEA_EINVAL, "NULL argument");
  if (const OptionDesc* d = find_option(name)) {
    *value = d->load(*h);
    return 0;
  }
  for (const ReadOnly& r : kReadOnly)
    if (std::strcmp(r.name, name) == 0) {
      const Part* p = h->parts.empty() ? nullptr : h->parts[0].get();
      if (r.part && !p) return fail(MFEA_ESTATE, std::string(name) + ": no partition yet");
      *value = r.get(h, p);
      return 0;
    }
  return fail(MFEA_EINVAL, std::string("unknown option ") + name);
}

int mfea_debug_option_info(int index, const char** name, int64_t* dflt, int* flags) {
  if (!name || !dflt || !flags) return fail(MFEA_EINVAL, "NULL argument");
  const int nw = option_count(), nr = (int)(sizeof kReadOnly / sizeof kReadOnly[0]);
  if (index < 0 || index >= nw + nr) return fail(MFEA_EINVAL, "option index out of range");
  if (index < nw) {
    const OptionDesc& d = option_at(index);
    *name = d.name;
    *dflt = option_default(d);
    *flags = MFEA_OPT_WRITABLE | (d.rebuilds_layout ? MFEA_OPT_REBUILDS_LAYOUT : 0) |
             (d.keeps_kept == OptKeeps::kYes ? MFEA_OPT_KEEPS_KEPT : 0);
  } else {
    *name = kReadOnly[index - nw].name;
    *dflt = 0;
    *flags = 0;
  }
  return 0;
}

int mfea_debug_global_active(mfea_handle* h, uint8_t* out) {
  if (!h || !out) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  RC(ensure_built(h));
  std::vector<uint8_t> key;
  if (partitioned(h)) RC(global_active(h, key));
  else RC(gather_active(h, key));
  std::copy(key.begin(), key.end(), out);
  return 0;
}

int mfea_debug_floating(mfea_handle* h, uint8_t* out) {
  if (!h || !out) return fail(MFEA_EINVAL, "bad argument");
  RC(set_device(h));
  RC(ensure_built(h));
  if (partitioned(h)) return fail(MFEA_ESTATE, "mfea_debug_floating: one partition");
  Part& pt = part0(h);
  const Pattern& P = pt.P;
  std::memset(out, 0, (size_t)h->N);
  if (P.n_free == 0) return 0;
  DevBuf<uint8_t> mask;
  HIPC(mask.alloc(P.n_free));
  HIPC(pt.cc_parent.alloc(std::max<int64_t>(P.n_nodes, 1)));
  HIPC(pt.cc_anch.alloc(std::max<int64_t>(P.n_nodes, 1)));
  launch_floating(h->stream, P.n_nodes, P.n_free, P.n_nodes - P.n_ghost, pt.slice_ptr.ptr, pt.row_len.ptr,
                  pt.s_col.ptr, pt.s_elem.ptr, pt.active.ptr, pt.cc_parent.ptr, pt.cc_anch.ptr, nullptr, mask.ptr,
                  h->opt_cc_tile);
  HIPC(hipGetLastError());
  std::vector<uint8_t> m(P.n_free);
  HIPC(hipMemcpyAsync(m.data(), mask.ptr, P.n_free, hipMemcpyDeviceToHost, h->stream));
  RC(sync_stream(h));
  for (int64_t r = 0; r < P.n_free; ++r) out[P.perm[r]] = m[r];
  return 0;
}

int mfea_debug_set_parts(mfea_handle* h, int nparts, int axis) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (nparts < 1 || nparts > kMaxRanks) return fail(MFEA_EINVAL, "nparts must be in [1, 64]");
  if (axis < -1 || axis > 1) return fail(MFEA_EINVAL, "axis must be -1, 0 or 1");
  if (h->world > 1 && nparts > 1) return fail(MFEA_ESTATE, "handle already joined an RCCL world");
  h->nparts = nparts;
  h->axis = axis;
  h->dirty = true;
  return 0;
}

int mfea_set_partition_axis(mfea_handle* h, int axis) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  if (axis < -1 || axis > 1) return fail(MFEA_EINVAL, "axis must be -1, 0 or 1");
  h->axis = axis;
  h->dirty = true;
  return 0;
}

int mfea_write_record_csv(const char* path, int style, int kind, int64_t n_rows, int64_t n_cols,
                          const double* values, const uint8_t* flags, int n_threads) {
  const std::string err =
      write_record_csv(path, style, kind, n_rows, n_cols, values, flags, n_threads);
  return err.empty() ? 0 : fail(MFEA_EINVAL, err);
}

int mfea_write_record_npy(const char* path, int kind, int64_t n_rows, int64_t n_cols, const double* values,
                          const uint8_t* flags) {
  const std::string err = write_record_npy(path, kind, n_rows, n_cols, values, flags);
  return err.empty() ? 0 : fail(MFEA_EINVAL, err);
}

int mfea_dist_unique_id(uint8_t* unique_id) {
  if (!unique_id) return fail(MFEA_EINVAL, "NULL argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId u;
  NCCLC(ncclGetUniqueId(&u));
  std::memcpy(unique_id, &u, sizeof(u));
  return 0;
}

int mfea_get_ownership(mfea_handle* h, uint8_t* node_owned, uint8_t* elem_owned) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  if (!partitioned(h)) {
    if (node_owned) std::memset(node_owned, 1, (size_t)h->N);
    if (elem_owned) std::memset(elem_owned, 1, (size_t)h->Ecount);
    return 0;
  }
  if (node_owned) std::memset(node_owned, 0, (size_t)h->N);
  if (elem_owned) std::memset(elem_owned, 0, (size_t)h->Ecount);
  for (auto& pp : h->parts) {
    const PartPlan& pl = pp->plan;
    if (node_owned)
      for (size_t ln = 0; ln < pl.node_g.size(); ++ln)
        if (!pl.ghost[ln]) node_owned[pl.node_g[ln]] = 1;
    if (elem_owned)
      for (size_t le = 0; le < pl.elem_g.size(); ++le)
        if (pl.elem_own[le]) elem_owned[pl.elem_g[le]] = 1;
  }
  return 0;
}

int mfea_gather_results(mfea_handle* h, double* U, double* stress, uint8_t* active) {
  if (!h) return fail(MFEA_EINVAL, "NULL handle");
  RC(set_device(h));
  RC(ensure_built(h));
  const int64_t N = h->N, E = h->Ecount;
  if (h->world <= 1) {
    if (U) RC(mfea_get_displacement(h, U));
    if (stress && E) RC(mfea_get_stress(h, stress));
    if (active && E) RC(mfea_get_active(h, active));
    return 0;
  }
  // this rank's values of its own nodes / elements (ascending global id);
  // every rank knows every rank's counts (the partition is deterministic)
  const int W = h->world, me = h->rank;
  std::vector<double> Ul(3 * N, 0.0), Sl(E, 0.0);
  std::vector<uint8_t> Al(E, 1), nown(N), eown(E);
  RC(mfea_get_displacement(h, Ul.data()));
  if (E) {
    RC(mfea_get_stress(h, Sl.data()));
    RC(mfea_get_active(h, Al.data()));
  }
  auto node_rank = [&](int64_t n) { return h->gowner[n]; };
  auto elem_rank = [&](int64_t e) {
    const int64_t a = h->e2n[2 * e], b = h->e2n[2 * e + 1];
    return (a < 0 || a >= N || b < 0 || b >= N) ? -1 : h->gowner[a];  // skipped elements: nobody's
  };
  std::vector<int64_t> len(W, 0), off(W + 1, 0);
  for (int64_t n = 0; n < N; ++n) len[node_rank(n)] += 3;
  for (int64_t e = 0; e < E; ++e)
    if (elem_rank(e) >= 0) len[elem_rank(e)] += 2;
  for (int p = 0; p < W; ++p) off[p + 1] = off[p] + len[p];
  hipStream_t s = h->stream;
  DevBuf<double> buf;
  if (me != 0) {
    std::vector<double> pk;
    pk.reserve(len[me]);
    for (int64_t n = 0; n < N; ++n)
      if (node_rank(n) == me)
        for (int a = 0; a < 3; ++a) pk.push_back(Ul[3 * n + a]);
    for (int64_t e = 0; e < E; ++e)
      if (elem_rank(e) == me) {
        pk.push_back(Sl[e]);
        pk.push_back(Al[e] ? 1.0 : 0.0);
      }
    HIPC(buf.alloc(pk.size() + 1));
    HIPC(hmemcpy(h, buf.ptr, pk.data(), pk.size() * sizeof(double), hipMemcpyHostToDevice));
    NCCLC(ncclGroupStart());
    if (!pk.empty()) NCCLC(ncclSend(buf.ptr, pk.size(), ncclFloat64, 0, h->comm, s));
    NCCLC(ncclGroupEnd());
    return sync_stream(h);
  }
  HIPC(buf.alloc(off[W] + 1));
  NCCLC(ncclGroupStart());
  for (int p = 1; p < W; ++p)
    if (len[p]) NCCLC(ncclRecv(buf.ptr + off[p], (size_t)len[p], ncclFloat64, p, h->comm, s));
  NCCLC(ncclGroupEnd());
  RC(sync_stream(h));
  std::vector<double> all(off[W]);
  if (off[W]) HIPC(hmemcpy(h, all.data(), buf.ptr, off[W] * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int64_t> at(off.begin(), off.end() - 1);
  for (int64_t n = 0; n < N; ++n) {
    const int p = node_rank(n);
    for (int a = 0; a < 3; ++a) {
      const double v = p == 0 ? Ul[3 * n + a] : all[at[p]++];
      if (U) U[3 * n + a] = v;
    }
  }
  for (int64_t e = 0; e < E; ++e) {
    const int p = elem_rank(e);
    double sv = Sl[e], av = Al[e];
    if (p > 0) {
      sv = all[at[p]++];
      av = all[at[p]++];
    }
    if (stress) stress[e] = sv;
    if (active) active[e] = av != 0.0 ? 1 : 0;
  }
  return 0;
}

int mfea_dist_init(mfea_handle* h, int rank, int world, const uint8_t* unique_id) {
  if (!h || !unique_id) return fail(MFEA_EINVAL, "NULL argument");
  if (world < 1 || world > kMaxRanks || rank < 0 || rank >= world)
    return fail(MFEA_EINVAL, "bad rank / world size");
  if (h->comm) return fail(MFEA_ESTATE, "handle already joined an RCCL world");
  if (h->nparts > 1) return fail(MFEA_ESTATE, "handle holds several partitions");
  RC(set_device(h));
  if (world > 1) {
    ncclUniqueId u;
    std::memcpy(&u, unique_id, sizeof(u));
    ncclComm_t c = nullptr;
    NCCLC(ncclCommInitRank(&c, world, u, rank));
    h->comm = c;
  }
  h->world = world;
  h->rank = rank;
  h->dirty = true;
  return 0;
}

}  // extern "C"
