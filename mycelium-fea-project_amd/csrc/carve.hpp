// carve.hpp — how many index arrays share one device int32 allocation: where
// each starts, how large the allocation is, and the list of copies that takes
// them there.  No HIP here: tests/native/carve_main.cpp compiles it alone;
// capi.hip's stage_begin allocates and stage_flush issues the copies.
#pragma once

#include <cstdint>
#include <vector>

namespace mfea {

constexpr size_t kAmgAlign = 64;  // elements: every carved array of the hierarchy starts 256/512-B aligned
inline size_t amg_al(size_t n) { return (n + kAmgAlign - 1) / kAmgAlign * kAmgAlign; }

// Arrays are placed one after the other: an array of n elements takes n + gap,
// rounded up to a multiple of align (1: none).  The hierarchy: kAmgAlign, no
// gap; the exchange plans: no rounding, a gap of 1 (so empty lists still get
// offsets of their own); the sweep and the halo: neither.  Two passes over the
// same calls: the first only counts (offsets and size() as the fill gives
// them); after begin_fill() the offsets start over and put(v) lists v for the
// copy — by address: v lives until the flush.  Pads and gaps are never
// written.  A fill that differs from the count ends with offset() != size().
class IndexStage {
 public:
  struct Item {
    size_t at;
    const std::vector<int32_t>* v;
  };
  explicit IndexStage(size_t align = 1, size_t gap = 0) : align_(align ? align : 1), gap_(gap) {}
  // the next array's offset
  size_t reserve(size_t n) {
    const size_t at = end_;
    end_ += (n + gap_ + align_ - 1) / align_ * align_;
    return at;
  }
  size_t put(const std::vector<int32_t>& v) {
    const size_t at = reserve(v.size());
    if (filling_ && !v.empty()) items_.push_back({at, &v});
    return at;
  }
  void begin_fill() {
    size_ = end_;
    end_ = 0;
    filling_ = true;
  }
  size_t size() const { return filling_ ? size_ : end_; }  // the counted total
  size_t offset() const { return end_; }                   // where the next array would start
  const std::vector<Item>& items() const { return items_; }

 private:
  size_t align_, gap_;
  size_t end_ = 0, size_ = 0;
  bool filling_ = false;
  std::vector<Item> items_;
};

}  // namespace mfea
