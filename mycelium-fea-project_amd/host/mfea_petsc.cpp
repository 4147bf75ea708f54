// mfea_petsc.cpp — command-line drop-in for the reference's PETSc executables
// (src/fea_petsc.cpp main(), src/fea_petsc_parallel.cpp at -np 1): the same
// `<results_dir>` argument, the same PETSc-style solver options, the same
// console lines and the same fea_results/*.csv dialect, with the hot path on
// the MI355X through libmfea.so (include/mfea.h).  Host C++ only: it reads the
// CSVs, makes the C-ABI calls and writes the records.
//
//   mfea_petsc <results_dir> [-ksp_type cg] [-pc_type icc|ilu|sor|jacobi|bjacobi|gamg]
//              [-ksp_rtol R] [-ksp_atol A] [-ksp_max_it N]
//              [-ksp_norm_type preconditioned|unpreconditioned]
//              [-n_steps N] [-disp_max D] [-grip_length G] [-max_strain S]
//              [-mfea_device K] [-mfea_reg R] [-grip_direction tx,ty,tz]
//
// -grip_direction: both grips move along (tx, ty, tz) instead of y, the ramp's
// displacements being the amplitudes (mfea_set_grip_motion; one process) — a
// shear or mixed-mode test; the force column is the work-conjugate force.
//
// Defaults are the reference's: its constants (src/fea_petsc.cpp:23-32) and
// PETSc's KSP defaults (rtol 1e-5, atol 1e-50, max_it 1e4, the preconditioned
// residual norm for CG).  The reference builds KSPCG with PCICC in source
// (src/fea_petsc.cpp:328-331) and PCBJACOBI in its MPI variant
// (src/fea_petsc_parallel.cpp:339): so does this driver — -pc_type icc is the
// default on one process, bjacobi under a multi-process launch.  icc (and ilu,
// the same factor of an SPD matrix) is the engine's IC(0) of the whole free
// system and sor its SSOR (ω = 1), both in a chain-piece multicolour order
// (sweep.hip; PETSc runs them in the natural order); bjacobi is the exact
// inverse of each node's 3×3 diagonal block and jacobi PCJACOBI.  Every
// preconditioner stops on PETSc's default CG norm, the preconditioned one,
// unless -ksp_norm_type unpreconditioned.  Documented differences: prescribed
// DOFs hold exactly their value (PETSc adds the 1e-12 shift to those rows too
// and returns x/(1+1e-12)); -pc_type gamg (the reference sweep's GAMG,
// src/fea_petsc_solverAndPC.cpp:330-391) is the engine's SA-AMG V-cycle;
// other -ksp_type are rejected.
//
// Multi-GPU: launched as N processes — `mpirun -np N mfea_petsc <dir>` as the
// reference's `mpirun -np 4 ./fea_petsc_parallel.exe` (README.md:18), or
// torch.distributed.run — every process takes its rank / size / local rank
// from the launcher's environment (OMPI_COMM_WORLD_*, PMI_*, RANK /
// WORLD_SIZE / LOCAL_RANK), drives the GPU of its local rank and joins the
// RCCL world (mfea_dist_init); rank 0 hands the communicator id to the others
// through a file (MFEA_UID_FILE, default <dir>/fea_results/.mfea_uid).
// Every rank solves its partition; rank 0 alone prints, gathers the records
// (mfea_gather_results) and writes the files — the reference has every rank
// write the same files (src/fea_petsc_parallel.cpp:491-574).
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <chrono>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mfea.h"

namespace {

struct Options {
  std::string dir;
  double rtol = 1e-5, atol = 1e-50, reg = 1e-12;
  int max_it = 10000;
  int precond = -1;  // -1: the reference's default (icc; bjacobi on several processes)
  int norm = MFEA_NORM_PRECONDITIONED;
  bool norm_given = false;
  int n_steps = 40;              // src/fea_petsc.cpp:28
  double disp_max = 0.02;        // :29
  double max_strain = 0.018;     // :30
  double grip = 1.5;             // :32
  int device = -1;
  bool grip_given = false;       // -grip_direction
  double grip_dir[3] = {0.0, 1.0, 0.0};
};

[[noreturn]] void die(const std::string& msg) {
  std::fprintf(stderr, "mfea_petsc: %s\n", msg.c_str());
  std::exit(1);
}

double num(const char* s, const char* opt) {
  char* end = nullptr;
  const double v = std::strtod(s, &end);
  if (!end || *end) die(std::string("bad value for ") + opt + ": " + s);
  return v;
}

Options parse(int argc, char** argv) {
  Options o;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a.empty() || a[0] != '-') {
      if (!o.dir.empty()) die("more than one results directory given");
      o.dir = a;
      continue;
    }
    if (i + 1 >= argc) die("option " + a + " needs a value");
    const char* v = argv[++i];
    if (a == "-ksp_type") {
      if (std::strcmp(v, "cg") != 0) die(std::string("-ksp_type ") + v + " not supported (cg only)");
    } else if (a == "-pc_type") {
      if (!std::strcmp(v, "jacobi")) o.precond = MFEA_PC_JACOBI;
      else if (!std::strcmp(v, "bjacobi")) o.precond = MFEA_PC_BLOCK_JACOBI;
      else if (!std::strcmp(v, "gamg")) o.precond = MFEA_PC_GAMG;
      else if (!std::strcmp(v, "icc") || !std::strcmp(v, "ilu")) o.precond = MFEA_PC_ICC;
      else if (!std::strcmp(v, "sor")) o.precond = MFEA_PC_SOR;
      else die(std::string("-pc_type ") + v + " not supported (icc, ilu, sor, jacobi, bjacobi, gamg)");
    } else if (a == "-ksp_norm_type") {
      o.norm_given = true;
      if (!std::strcmp(v, "preconditioned")) o.norm = MFEA_NORM_PRECONDITIONED;
      else if (!std::strcmp(v, "unpreconditioned")) o.norm = MFEA_NORM_UNPRECONDITIONED;
      else die(std::string("-ksp_norm_type ") + v + " not supported");
    } else if (a == "-ksp_rtol") {
      o.rtol = num(v, "-ksp_rtol");
    } else if (a == "-ksp_atol") {
      o.atol = num(v, "-ksp_atol");
    } else if (a == "-ksp_max_it") {
      o.max_it = (int)num(v, "-ksp_max_it");
    } else if (a == "-n_steps") {
      o.n_steps = (int)num(v, "-n_steps");
    } else if (a == "-disp_max") {
      o.disp_max = num(v, "-disp_max");
    } else if (a == "-grip_length") {
      o.grip = num(v, "-grip_length");
    } else if (a == "-max_strain") {
      o.max_strain = num(v, "-max_strain");
    } else if (a == "-mfea_device") {
      o.device = (int)num(v, "-mfea_device");
    } else if (a == "-mfea_reg") {
      o.reg = num(v, "-mfea_reg");
    } else if (a == "-grip_direction") {
      std::stringstream ss(v);
      std::string f;
      int n = 0;
      while (std::getline(ss, f, ',')) {
        if (n == 3) die(std::string("-grip_direction needs three components: ") + v);
        o.grip_dir[n++] = num(f.c_str(), "-grip_direction");
      }
      if (n != 3) die(std::string("-grip_direction needs three components: ") + v);
      for (double c : o.grip_dir)
        if (!std::isfinite(c)) die(std::string("-grip_direction must be finite: ") + v);
      if (o.grip_dir[0] == 0.0 && o.grip_dir[1] == 0.0 && o.grip_dir[2] == 0.0)
        die("-grip_direction must not be all zero");
      o.grip_given = true;
    } else {
      die("unknown option " + a);
    }
  }
  if (o.n_steps < 2) die("-n_steps must be at least 2");
  return o;
}

// the preconditioner default (the reference's PCICC; its MPI variant's
// PCBJACOBI).  Every preconditioner stops on PETSc's default KSPCG norm, the
// preconditioned one, unless -ksp_norm_type says otherwise
// (src/fea_petsc.cpp:336-341).
void finish_options(Options& o, int world) {
  if (o.precond < 0) o.precond = world > 1 ? MFEA_PC_BLOCK_JACOBI : MFEA_PC_ICC;
  if (world > 1 && (o.precond == MFEA_PC_ICC || o.precond == MFEA_PC_SOR))
    die("-pc_type icc / ilu / sor: one process (use bjacobi, jacobi or gamg under mpirun)");
  if (world > 1 && o.grip_given) die("-grip_direction: one process");
}

// src/fea_petsc.cpp:42-82: header skipped, empty lines skipped, the first
// 4 (nodes) / 3 (elements) comma fields through stoi / stod; row order = index.
void read_nodes(const std::string& path, std::vector<double>& xyz) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("Failed to open nodes file: " + path);
  std::string line, tok;
  std::getline(f, line);
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::stringstream ss(line);
    std::getline(ss, tok, ',');
    (void)std::stoi(tok);
    for (int c = 0; c < 3; ++c) {
      std::getline(ss, tok, ',');
      xyz.push_back(std::stod(tok));
    }
  }
}

void read_elems(const std::string& path, std::vector<int64_t>& e2n) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error("Failed to open elements file: " + path);
  std::string line, tok;
  std::getline(f, line);
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::stringstream ss(line);
    std::getline(ss, tok, ',');
    (void)std::stoi(tok);
    for (int c = 0; c < 2; ++c) {
      std::getline(ss, tok, ',');
      e2n.push_back(std::stoi(tok));
    }
  }
}

// rank, world size, local rank of a multi-process launch (else 0, 1, -1)
struct Launch {
  int rank = 0, world = 1, local = -1;
};
int env_int(const char* const* names, int dflt) {
  for (int k = 0; names[k]; ++k)
    if (const char* v = std::getenv(names[k])) return std::atoi(v);
  return dflt;
}
Launch launch_env() {
  static const char* const rank[] = {"OMPI_COMM_WORLD_RANK", "PMI_RANK", "RANK", nullptr};
  static const char* const size[] = {"OMPI_COMM_WORLD_SIZE", "PMI_SIZE", "WORLD_SIZE", nullptr};
  static const char* const local[] = {"OMPI_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID", "LOCAL_RANK", nullptr};
  Launch l;
  l.rank = env_int(rank, 0);
  l.world = env_int(size, 1);
  l.local = env_int(local, -1);
  return l;
}

// Rank 0 writes the 128-byte RCCL id to `path` (temp file + rename: readers
// never see a partial file); the others wait for a file no older than their
// own start (a previous run's file is ignored), up to 120 s.
void exchange_uid(const Launch& l, const std::string& path, uint8_t* uid,
                  std::chrono::system_clock::time_point started) {
  if (l.rank == 0) {
    if (mfea_dist_unique_id(uid) != MFEA_OK) die("mfea_dist_unique_id failed");
    const std::string tmp = path + ".tmp";
    std::FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f || std::fwrite(uid, 1, 128, f) != 128 || std::fclose(f) != 0) die("cannot write " + tmp);
    if (std::rename(tmp.c_str(), path.c_str()) != 0) die("cannot create " + path);
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const auto since = std::chrono::system_clock::to_time_t(started) - 5;
  for (;;) {
    struct stat st;
    if (stat(path.c_str(), &st) == 0 && st.st_mtime >= since && st.st_size == 128) {
      std::FILE* f = std::fopen(path.c_str(), "rb");
      const bool ok = f && std::fread(uid, 1, 128, f) == 128;
      if (f) std::fclose(f);
      if (ok) return;
    }
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
      die("rank " + std::to_string(l.rank) + ": no communicator id from rank 0 in " + path);
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
}

std::string last_error() {
  char buf[512];
  mfea_last_error(buf, sizeof(buf));
  return buf;
}

void check(int rc, const char* what) {
  if (rc != MFEA_OK) die(std::string(what) + ": " + last_error());
}

void write(const std::string& path, int kind, int64_t rows, int64_t cols, const double* v,
           const uint8_t* f) {
  if (mfea_write_record_csv(path.c_str(), MFEA_CSV_PETSC, kind, rows, cols, v, f, 16) != MFEA_OK)
    die(last_error());
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("Usage: %s <results_dir>\n", argv[0]);
    return 1;
  }
  Options o = parse(argc, argv);
  if (o.dir.empty()) {
    std::printf("Usage: %s <results_dir>\n", argv[0]);
    return 1;
  }
  const auto started = std::chrono::system_clock::now();
  const Launch L = launch_env();
  if (L.world < 1 || L.rank < 0 || L.rank >= L.world) die("bad rank / world size in the environment");
  finish_options(o, L.world);
  const bool root = L.rank == 0;
  const std::string fea_dir = o.dir + "/fea_results";
  struct stat st;
  if (stat(fea_dir.c_str(), &st) != 0) mkdir(fea_dir.c_str(), 0755);
  if (root) std::printf("🔧 Running FEA on geometry from %s\n", o.dir.c_str());
  const auto t_start = std::chrono::high_resolution_clock::now();

  std::vector<double> xyz;
  std::vector<int64_t> e2n;
  try {
    read_nodes(o.dir + "/nodes.csv", xyz);
    read_elems(o.dir + "/elements.csv", e2n);
  } catch (const std::exception& ex) {
    std::printf("Error reading input CSVs: %s\n", ex.what());
    return 1;
  }
  const int64_t N = (int64_t)xyz.size() / 3, E = (int64_t)e2n.size() / 2, n_dof = 3 * N;
  if (N == 0) {
    std::printf("Error reading input CSVs: no nodes\n");
    return 1;
  }
  // grips by row index, src/fea_petsc.cpp:203-213
  double y_min = xyz[1], y_max = xyz[1];
  for (int64_t i = 1; i < N; ++i) {
    y_min = std::min(y_min, xyz[3 * i + 1]);
    y_max = std::max(y_max, xyz[3 * i + 1]);
  }
  std::vector<int64_t> top, bot;
  for (int64_t i = 0; i < N; ++i) {
    if (std::fabs(xyz[3 * i + 1] - y_max) < o.grip) top.push_back(i);
    if (std::fabs(xyz[3 * i + 1] - y_min) < o.grip) bot.push_back(i);
  }
  if (root) std::printf("Top nodes: %zu, Bottom nodes: %zu\n", top.size(), bot.size());

  int device = o.device;
  if (device < 0) device = L.local >= 0 ? L.local : 0;
  mfea_handle* h = nullptr;
  check(mfea_create(device, &h), "mfea_create");
  if (L.world > 1) {
    const char* uf = std::getenv("MFEA_UID_FILE");
    uint8_t uid[128];
    exchange_uid(L, uf ? std::string(uf) : fea_dir + "/.mfea_uid", uid, started);
    check(mfea_dist_init(h, L.rank, L.world, uid), "mfea_dist_init");
  }
  if (o.grip_given) check(mfea_set_grip_motion(h, o.grip_dir, o.grip_dir), "mfea_set_grip_motion");
  // out-of-range node ids are skipped, as src/fea_petsc.cpp:241 does
  check(mfea_set_mesh(h, N, xyz.data(), E, e2n.data(), MFEA_MESH_SKIP_INVALID), "mfea_set_mesh");
  check(mfea_set_bc(h, (int64_t)top.size(), top.data(), (int64_t)bot.size(), bot.data()),
        "mfea_set_bc");
  check(mfea_set_active(h, nullptr), "mfea_set_active");
  mfea_solve_opts so;
  so.rtol = o.rtol;
  so.atol = o.atol;
  so.max_it = o.max_it;
  so.precond = o.precond;
  so.norm = o.norm;
  so.chunk = 0;
  so.reg = o.reg;

  std::vector<double> stress_rec, disp_rec, fd;
  std::vector<uint8_t> active_rec;
  std::vector<double> U(n_dof), S(E);
  std::vector<uint8_t> A(E);
  int64_t steps = 0;
  for (int step = 0; step < o.n_steps; ++step) {
    const double f = (double)step / (double)(o.n_steps - 1);
    const double dy_top = +o.disp_max * f, dy_bot = -o.disp_max * f;
    if (root) std::printf("➡️  Step %d/%d | dy_top=%.6f, dy_bot=%.6f\n", step + 1, o.n_steps, dy_top, dy_bot);
    double force = 0.0;
    int64_t n_active = 0;
    mfea_stats stt;
    const int rc = mfea_step(h, dy_top, dy_bot, &so, o.max_strain, &force, &n_active, &stt);
    if (rc == MFEA_EMAXIT || rc == MFEA_EBREAKDOWN) {
      // KSPConvergedReason: KSP_DIVERGED_ITS = -3, KSP_DIVERGED_BREAKDOWN = -5
      if (root)
        std::printf("❌ Solver failed to converge at step %d. Reason %d\n", step + 1, rc == MFEA_EMAXIT ? -3 : -5);
      break;
    }
    check(rc, "mfea_step");
    // KSP_CONVERGED_RTOL = 2, KSP_CONVERGED_ATOL = 3 (a zero right-hand side)
    const int reason = stt.bnorm == 0.0 ? 3 : 2;
    if (root) {
      std::printf("KSP converged reason: %d\n", reason);
      std::printf("KSP Object: %d MPI process%s (mfea, device %d)\n  type: cg, %d iterations, "
                  "final relative residual %.3e\n  tolerances: relative=%g, absolute=%g, "
                  "maximum iterations=%d\n  using %s norm type for convergence test\n"
                  "PC Object: type %s\n",
                  L.world, L.world > 1 ? "es" : "", device, stt.iters, stt.relres, o.rtol, o.atol, o.max_it,
                  o.norm == MFEA_NORM_PRECONDITIONED ? "PRECONDITIONED" : "UNPRECONDITIONED",
                  o.precond == MFEA_PC_JACOBI ? "jacobi" : o.precond == MFEA_PC_GAMG ? "gamg"
                  : o.precond == MFEA_PC_ICC ? "icc (DIC(0) of the whole matrix, chain-piece multicolour order)"
                  : o.precond == MFEA_PC_SOR ? "sor (SSOR of the whole matrix, chain-piece multicolour order)"
                  : "bjacobi (3x3 node blocks)");
    }
    // the whole mesh's records on rank 0 (collective; one process: a copy)
    check(mfea_gather_results(h, U.data(), E ? S.data() : nullptr, E ? A.data() : nullptr), "mfea_gather_results");
    if (!root) {
      if (n_active == 0) break;
      continue;
    }
    fd.push_back(dy_top - dy_bot);
    fd.push_back(force);
    disp_rec.insert(disp_rec.end(), U.begin(), U.end());
    stress_rec.insert(stress_rec.end(), S.begin(), S.end());
    active_rec.insert(active_rec.end(), A.begin(), A.end());
    ++steps;
    if (n_active == 0) {
      std::printf("⚠️  Simulation stopped early at step %d.\n", step + 1);
      break;
    }
  }
  mfea_destroy(h);
  if (!root) return 0;

  // src/fea_petsc.cpp:433-516: a record file is written when it holds a step
  if (steps) {
    write(fea_dir + "/stress_record.csv", MFEA_REC_STRESS, steps, E, stress_rec.data(), nullptr);
    write(fea_dir + "/active_elements.csv", MFEA_REC_ACTIVE, steps, E, nullptr, active_rec.data());
    write(fea_dir + "/node_displacements.csv", MFEA_REC_DISP, steps, n_dof, disp_rec.data(), nullptr);
    write(fea_dir + "/force_displacement.csv", MFEA_REC_FORCE, steps, 2, fd.data(), nullptr);
  }
  {
    std::ofstream rt(fea_dir + "/runtime.txt");
    rt << "FEA run finished (no timing collected inside C++ version).\n";
  }
  std::printf("✅ FEA completed. Results saved to %s\n", fea_dir.c_str());
  const auto t_stop = std::chrono::high_resolution_clock::now();
  const auto us = std::chrono::duration_cast<std::chrono::microseconds>(t_stop - t_start);
  std::cout << "Time taken by myLongRunningFunction: " << us.count() << " microseconds" << std::endl;
  return 0;
}
