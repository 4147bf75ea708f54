// fuse_shim.cpp — TEST-ONLY C entry points over level 0's sorting window
// (amg.hpp AmgLayout::l0_window) and the block halo plan (AmgFusePlan) of the
// host symbolic phase.  Built on host_shim.cpp's entry points (same pattern,
// same plan object), so tests/amg_ref.py fetches its plans as it does there.
#include "host_shim.cpp"

extern "C" {

// level 0's window of the next shim_amg (rows, a multiple of 64)
void shim_amg_l0_window(int64_t rows) { g_layout.l0_window = rows; }
int64_t shim_amg_l0_window_used() { return g_amg.l0_window; }

// plan arrays shim_amg_array does not export
int64_t shim_amg_array_more(int l, const char* name, int32_t* out) {
  const std::string n(name);
  if (l < 0 || l >= (int)g_amg.lev.size()) return -1;
  const AmgLevel& L = g_amg.lev[l];
  const std::vector<int32_t>* v = nullptr;
  if (n == "nat") v = &L.nat;
  else if (n == "A.rlen") v = &L.A.rlen;
  else if (n == "P.rlen") v = &L.P.rlen;
  else if (n == "R.rlen") v = &L.R.rlen;
  else if (n == "AP.rlen") v = &L.AP.rlen;
  else if (n == "PT.rlen") v = &L.PT.rlen;
  else if (n == "RT.rlen") v = &L.RT.rlen;
  else return -1;
  if (out) std::memcpy(out, v->data(), v->size() * 4);
  return (int64_t)v->size();
}

static AmgFusePlan g_fuse;
// the halo plan of the last shim_amg plan: 1 on, 0 off, -1 error;
// info = [B, n_blocks, max_halo, cut, offdiag]
int shim_fuse(int64_t halo_cap, int64_t* info, char* err, int errn) {
  const std::string e = build_amg_fuse(g_amg, halo_cap, g_fuse);
  if (!e.empty()) {
    std::snprintf(err, errn, "%s", e.c_str());
    return -1;
  }
  std::snprintf(err, errn, "%s", g_fuse.why.c_str());
  info[0] = g_fuse.B;
  info[1] = g_fuse.n_blocks;
  info[2] = g_fuse.max_halo;
  info[3] = g_fuse.cut;
  info[4] = g_fuse.offdiag;
  return g_fuse.on ? 1 : 0;
}
// hptr / hrow / hpt (int32) and lcol (widened to int32, 0xFFFF → 65535)
int64_t shim_fuse_array(const char* name, int32_t* out) {
  const std::string n(name);
  if (n == "lcol") {
    if (out)
      for (size_t k = 0; k < g_fuse.lcol.size(); ++k) out[k] = (int32_t)g_fuse.lcol[k];
    return (int64_t)g_fuse.lcol.size();
  }
  const std::vector<int32_t>* v = nullptr;
  if (n == "hptr") v = &g_fuse.hptr;
  else if (n == "hrow") v = &g_fuse.hrow;
  else if (n == "hpt") v = &g_fuse.hpt;
  else return -1;
  if (out) std::memcpy(out, v->data(), v->size() * 4);
  return (int64_t)v->size();
}
}  // extern "C"
