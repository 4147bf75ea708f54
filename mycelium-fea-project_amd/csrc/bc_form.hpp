// bc_form.hpp — the boundary forms of the RHS, reaction and event kernels, and
// the one place that chooses between them.  Host-only, no HIP header: plain
// g++ compiles it alone (tests/native/bc_form_main.cpp).
//
// The kernels are templates over a grip form GM and a load form LD, with no
// run-time choice inside them.  A launcher takes a BcForm and hands its launch
// to with_grip / with_bc, which call it with the forms' values; the callable
// names the instantiation by decltype.  A new form is one more rung here plus
// its kernel bodies.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <stdint.h>
#include <vector>

namespace mfea {

// Grip motion (mfea_set_grip_motion): the prescribed displacement of a grip
// node is amplitude · direction, p[c] = fl(dy · dir[c]) — one f64 product per
// component, formed once per launch (device_util.hpp grip_disp).  GripY: the
// tensile test, (0, dy, 0) — the kernels as they were before the directions
// existed.  GripVec: any two directions; a free row's RHS then takes the whole
// symmetric block of a known neighbour, b −= V·p, and a known row x = p.
// GripField (mfea_set_grip_field): a vector per grip node instead of one per
// band — d holds 3 doubles per known row in Pattern row order, row j at
// d[3·(j − nf)], and the prescribed displacement of row j is
// p[c] = fl(amp · d[3·(j − nf) + c]) with amp the amplitude of the row's class
// (dy_bot for a bottom row, dy_top for a top row).  The RHS term and the known
// rows' x are GripVec's with p per row.
struct GripY {};
struct GripVec {
  double top[3], bot[3];
};
struct GripField {
  const double* d;
};

// Nodal loads (mfea_set_node_loads): the load policy beside the grip policy.
// LoadNone: b = 0 − K_fk x_k, the kernels as they were before loads existed.
// NodeLoad: a free row r takes b[c] = q[c] − k[c], k the grip term accumulated
// as without loads and
//   q[c] = fl(amp · f[3r + c]) + 0,  amp = dy_top (prop) or 1 (a dead load:
//   the product is the stored value), 0 where fl[r] is set
// f: 3 doubles per free row in Pattern row order; fl: a byte per free row, 1 on
// the rows of floating pieces (launch_floating's mask in row order) — their
// load is dropped, so they stay at exactly zero.  (+ 0: a product −0 counts as
// 0, as a stored −0 does; with f = 0 the bits are LoadNone's.)
struct LoadNone {};
struct NodeLoad {
  const double* f;
  const uint8_t* fl;
  int32_t prop;
};

// What a launcher is told: null is the default form (GripY, LoadNone); field
// takes precedence over grip.  The pointers are read during the call only.
struct BcForm {
  const GripVec* grip;
  const double* field;
  const NodeLoad* load;
};

// f(GripField{field}), f(*grip) or f(GripY{}) — the precedence is decided here
// and nowhere else
template <class F>
void with_grip(const BcForm& bc, F&& f) {
  if (bc.field) f(GripField{bc.field});
  else if (bc.grip) f(*bc.grip);
  else f(GripY{});
}
// f(gm, ld): gm as with_grip passes it, ld = *load or LoadNone{}
template <class F>
void with_bc(const BcForm& bc, F&& f) {
  with_grip(bc, [&](auto gm) {
    if (bc.load) f(gm, *bc.load);
    else f(gm, LoadNone{});
  });
}

// A vector per node in the caller's node order, as mfea_set_grip_field and
// mfea_set_node_loads keep it on the host: 3 doubles per node while set.
struct NodeVectors {
  std::vector<double> v;
  bool set = false;
  // a z component anywhere (entries 2, 5, 8, …): the solution leaves the plane
  bool z() const {
    for (size_t n = 2; n < v.size(); n += 3)
      if (v[n] != 0.0) return true;
    return false;
  }
  void reset() {
    v.clear();
    set = false;
  }
};
enum class VecStage { kNotFinite, kSame, kNew };
// src (n doubles, or null: unset) checked and normalised into staged: every
// entry finite, a −0 entry stored as 0.  kSame: cur holds exactly this state,
// byte for byte; kNew: NodeVectors::v.swap(staged) and set = (src != null)
// make it the state.
inline VecStage stage_node_vectors(const NodeVectors& cur, const double* src, size_t n,
                                   std::vector<double>& staged) {
  staged.clear();
  if (src) {
    staged.resize(n);
    for (size_t k = 0; k < n; ++k) {
      if (!std::isfinite(src[k])) return VecStage::kNotFinite;
      staged[k] = src[k] + 0.0;
    }
  }
  if (cur.set != (src != nullptr)) return VecStage::kNew;
  if (!src || n == 0) return VecStage::kSame;
  return cur.v.size() == n && std::memcmp(staged.data(), cur.v.data(), n * sizeof(double)) == 0 ? VecStage::kSame
                                                                                                 : VecStage::kNew;
}

}  // namespace mfea
