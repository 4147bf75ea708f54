// Stand-alone driver of csrc/bc_form.hpp for tests/test_bc_form_cpu.py (host
// C++ only).  Commands on stdin, one per line; doubles travel as the hex of
// their bits, so NaN, ±inf and −0 arrive as written:
//   form G F L          with_bc and with_grip on a BcForm whose grip / field /
//                       load pointer is non-null where the flag is 1
//     → "bc <calls> <GM> <LD> <payload>" and "grip <calls> <GM> <payload>"
//   stage S m c.. Q n x..   stage_node_vectors: the current state (S: set, m
//                       entries c), the source (Q = 0: null, n entries x)
//     → "stage <notfinite|same|new> <staged entries>"
//   z m c..             NodeVectors::z of m entries → "z <0|1>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "bc_form.hpp"

using namespace mfea;

static const GripVec kGrip{{1.5, -2.0, 3.25}, {-4.0, 5.5, 6.0}};
static const double kField[3] = {7.0, 8.0, 9.0};
static const double kLoadF[3] = {10.0, 11.0, 12.0};
static const uint8_t kMask[1] = {1};
static const NodeLoad kLoad{kLoadF, kMask, 7};

static std::string show(GripY) { return "GripY -"; }
static std::string show(const GripVec& g) {
  return std::string("GripVec ") + (std::memcmp(&g, &kGrip, sizeof g) == 0 ? "same" : "differs");
}
static std::string show(GripField f) { return std::string("GripField ") + (f.d == kField ? "same" : "differs"); }
static std::string show(LoadNone) { return "LoadNone -"; }
static std::string show(const NodeLoad& l) {
  return std::string("NodeLoad ") + (l.f == kLoadF && l.fl == kMask && l.prop == 7 ? "same" : "differs");
}

static double from_bits(const std::string& hex) {
  const uint64_t u = std::stoull(hex, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}
static std::vector<double> read_vec(std::istringstream& in) {
  size_t n = 0;
  in >> n;
  std::vector<double> v(n);
  std::string t;
  for (size_t k = 0; k < n; ++k) {
    in >> t;
    v[k] = from_bits(t);
  }
  return v;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "form") {
      int g = 0, f = 0, l = 0;
      in >> g >> f >> l;
      const BcForm bc{g ? &kGrip : nullptr, f ? kField : nullptr, l ? &kLoad : nullptr};
      int calls = 0;
      std::string gm, ld;
      with_bc(bc, [&](auto a, auto b) {
        ++calls;
        gm = show(a);
        ld = show(b);
      });
      std::printf("bc %d %s %s\n", calls, gm.c_str(), ld.c_str());
      calls = 0;
      with_grip(bc, [&](auto a) {
        ++calls;
        gm = show(a);
      });
      std::printf("grip %d %s\n", calls, gm.c_str());
    } else if (cmd == "stage") {
      NodeVectors cur;
      int set = 0, given = 0;
      in >> set;
      cur.set = set != 0;
      cur.v = read_vec(in);
      in >> given;
      // (a copy of exactly n entries on the heap: a read past either end is the sanitizer's)
      const std::vector<double> src = read_vec(in);
      std::vector<double> staged;
      static const double kNone = 0.0;  // (an empty vector's data() may be null: a given array of no entries)
      const double* p = !given ? nullptr : src.empty() ? &kNone : src.data();
      const VecStage st = stage_node_vectors(cur, p, src.size(), staged);
      std::printf("stage %s", st == VecStage::kNotFinite ? "notfinite" : st == VecStage::kSame ? "same" : "new");
      if (st != VecStage::kNotFinite)
        for (const double d : staged) {
          uint64_t u;
          std::memcpy(&u, &d, sizeof u);
          std::printf(" %016" PRIx64, u);
        }
      std::printf("\n");
    } else if (cmd == "z") {
      NodeVectors nv;
      nv.v = read_vec(in);
      nv.set = true;
      std::printf("z %d\n", nv.z() ? 1 : 0);
      nv.reset();
      if (nv.set || !nv.v.empty() || nv.z()) return 3;
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
