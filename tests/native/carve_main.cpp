// Stand-alone driver of csrc/carve.hpp (host code only; built by
// tests/test_carve_cpu.py, with the sanitizers).  Every stdin line is one case,
// "align gap item_0 item_1 ...": item k is a length n — a vector that holds
// (k + 1) * 100000 + i + 1 at i (never zero), put — or rn: n elements
// reserved.  A sizing pass counts them; the fill pass places them again, and
// the stage's copy list is applied (memcpy standing in for the device copy)
// to memory of exactly the counted size that held -1 everywhere.  Three lines
// come out: "sized end size" (the sizing pass's total, the fill's end offset,
// size() after it), the offsets, the memory.  First of all, one line "overrun
// <end> <size>": a fill that places more than was counted.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "carve.hpp"

using namespace mfea;

int main() {
  {
    const std::vector<int32_t> three(3, 1), two(2, 1);
    IndexStage st(1, 0);
    st.put(three);
    st.begin_fill();
    st.put(two);
    st.put(two);
    std::printf("overrun %zu %zu\n", st.offset(), st.size());
  }
  char buf[1 << 16];
  while (std::fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    size_t align, gap;
    std::string item;
    if (!(in >> align >> gap)) continue;
    std::vector<std::vector<int32_t>> vs;
    std::vector<bool> only_reserved;
    while (in >> item) {
      const bool r = item[0] == 'r';
      std::vector<int32_t> v(std::stoul(item.substr(r ? 1 : 0)));
      for (size_t i = 0; i < v.size(); ++i) v[i] = (int32_t)((vs.size() + 1) * 100000 + i + 1);
      vs.push_back(v);
      only_reserved.push_back(r);
    }
    IndexStage st(align, gap);
    auto place = [&](size_t k) { return only_reserved[k] ? st.reserve(vs[k].size()) : st.put(vs[k]); };
    for (size_t k = 0; k < vs.size(); ++k) place(k);
    const size_t sized = st.size();
    if (!st.items().empty()) return 1;  // (a sizing pass lists nothing)
    st.begin_fill();
    std::vector<size_t> off;
    for (size_t k = 0; k < vs.size(); ++k) off.push_back(place(k));
    std::vector<int32_t> mem(sized, -1);
    for (const IndexStage::Item& it : st.items()) {
      if (it.at + it.v->size() > mem.size()) return 1;
      std::memcpy(mem.data() + it.at, it.v->data(), it.v->size() * sizeof(int32_t));
    }
    std::printf("%zu %zu %zu\n", sized, st.offset(), st.size());
    for (size_t o : off) std::printf("%zu ", o);
    std::printf("\n");
    for (int32_t x : mem) std::printf("%d ", x);
    std::printf("\n");
  }
  return 0;
}
