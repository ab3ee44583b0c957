// prad_sweep_plan.h -- what a segment-mode GLCM / GLRLM call runs on the sweep kernels: the plan (table sizes, workgroups per
// role, piece lengths, LDS bytes) as a pure function of the call's shape, the switches and the compute-unit count.
// No Call, no Context, no HIP call: prad_debug_sweep_plan records its result and tests/test_sweep_plan.py holds it to
// tests/golden/sweep_plans.npz.  The table layouts it sizes (SweepSet, FwSet, hist_layout, ...) are those of the kernel headers.
//
// sweep_knobs_from_env() is the ONLY place of the GLCM / GLRLM route that reads the environment (DESIGN.md lists the switches).
#pragma once
#include "kernels_sweepfw2.h"   // (and through it kernels_sweepfw.h and kernels_sweep.h)

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace prad {
#pragma GCC visibility push(hidden)   // (the library exports the C ABI only)

// ---- the switches ---------------------------------------------------------------------------------------------------------
struct Knob {          // an override that may be absent
  bool set = false;
  long long v = 0;
};
struct SweepKnobs {
  // planner: routes taken out (baselines and checkers) ...
  bool no_fw = false;          // PRAD_NO_FW: no fixed-window kernel (fused table)
  bool no_fw2 = false;         // PRAD_NO_FW2: no two-table fixed-window kernel
  bool no_fw2_rows = false;    // PRAD_NO_FW2_ROWS: the x angle of a two-table volume on the rows kernel of kernels_sweep.h
  bool fw2_noskip1 = false;    // PRAD_FW2_NOSKIP1: the two-table walk records its runs of length 1
  bool fw_xrole_off = false;   // PRAD_FW_XROLE=0: the x angle as a launch of its own (checker of the trailing role)
  // ... and tuning overrides
  Knob threads, lpl, lines_blocks;                                                  // PRAD_THREADS, PRAD_LPL, PRAD_LINES_BLOCKS
  Knob fw2_copies, fw2_rs, fw2_rows_waves;                                          // PRAD_FW2_COPIES, PRAD_FW2_RS, PRAD_FW2_ROWS_WAVES
  Knob fw_budget_kb, fw_rs, fw_blocks, fw_threads, fw_per_wave, fw_cl, fw_xcd;      // PRAD_FW_BUDGET_KB, ... , PRAD_FW_XCD
  Knob fw_rows_threads, fw_xblocks, fw_xgpd;                                        // PRAD_FW_ROWS_THREADS, PRAD_FW_XBLOCKS, PRAD_FW_XGPD
  // pack cadence
  Knob pack_every;             // PRAD_PACK_EVERY
  // pipeline
  bool fin_ride = true;        // PRAD_FIN_RIDE=0: finalize and zeroing as launches of their own (checker of the riding job)
  bool finalize_one = true;    // PRAD_FINALIZE_ONE=0: the three finalize launches (checker of finalize_volume_kernel)
  bool no_inline_pack = false; // PRAD_NO_INLINE_PACK: every pack a launch of its own (baseline)
  bool no_pairs = false;       // PRAD_NO_PAIRS: no pairs tier between the sweeps and the exact kernels (baseline)
  bool lanes_mode = false;     // PRAD_DEFERRED_MODE=lanes
  int pipe_twin = -1;          // PRAD_PIPE_TWIN: 1 = deal pipeline volumes onto two pipelines on two internal streams, 0 = one
                               // pipeline on the caller's stream, unset (-1) = by volume size (prad_pipe_plan.h kTwinMinVoxels)
};

inline Knob env_knob(const char *name, bool wide = false) {
  Knob k;
  if (const char *e = getenv(name)) {
    k.set = true;
    k.v = wide ? atoll(e) : (long long)atoi(e);
  }
  return k;
}
// "NAME=0" switches something off that is on by default; unset, empty or anything else leaves it on
inline bool env_not_zero(const char *name) {
  const char *e = getenv(name);
  return !(e && atoi(e) == 0 && e[0] != '\0');
}

inline SweepKnobs sweep_knobs_from_env() {
  SweepKnobs k;
  k.no_fw = getenv("PRAD_NO_FW") != nullptr;
  k.no_fw2 = getenv("PRAD_NO_FW2") != nullptr;
  k.no_fw2_rows = getenv("PRAD_NO_FW2_ROWS") != nullptr;
  k.fw2_noskip1 = getenv("PRAD_FW2_NOSKIP1") != nullptr;
  {
    const char *e = getenv("PRAD_FW_XROLE");
    k.fw_xrole_off = e && atoi(e) == 0;
  }
  k.threads = env_knob("PRAD_THREADS");
  k.lpl = env_knob("PRAD_LPL");
  k.lines_blocks = env_knob("PRAD_LINES_BLOCKS");
  k.fw2_copies = env_knob("PRAD_FW2_COPIES");
  k.fw2_rs = env_knob("PRAD_FW2_RS", true);
  k.fw2_rows_waves = env_knob("PRAD_FW2_ROWS_WAVES");
  k.fw_budget_kb = env_knob("PRAD_FW_BUDGET_KB");
  k.fw_rs = env_knob("PRAD_FW_RS");
  k.fw_blocks = env_knob("PRAD_FW_BLOCKS");
  k.fw_threads = env_knob("PRAD_FW_THREADS");
  k.fw_per_wave = env_knob("PRAD_FW_PER_WAVE");
  k.fw_cl = env_knob("PRAD_FW_CL");
  k.fw_xcd = env_knob("PRAD_FW_XCD");
  k.fw_rows_threads = env_knob("PRAD_FW_ROWS_THREADS");
  k.fw_xblocks = env_knob("PRAD_FW_XBLOCKS", true);
  k.fw_xgpd = env_knob("PRAD_FW_XGPD");
  k.pack_every = env_knob("PRAD_PACK_EVERY");
  k.fin_ride = env_not_zero("PRAD_FIN_RIDE");
  k.finalize_one = env_not_zero("PRAD_FINALIZE_ONE");
  k.no_inline_pack = getenv("PRAD_NO_INLINE_PACK") != nullptr;
  k.no_pairs = getenv("PRAD_NO_PAIRS") != nullptr;
  {
    const char *e = getenv("PRAD_DEFERRED_MODE");
    k.lanes_mode = e && strcmp(e, "lanes") == 0;
  }
  {
    const char *e = getenv("PRAD_PIPE_TWIN");
    k.pipe_twin = (e && e[0] != '\0') ? (atoi(e) != 0 ? 1 : 0) : -1;
  }
  return k;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------
struct SweepPlan {
  bool ok = false;
  int Nz = 1, Ny = 1, Nx = 1;  // volume embedded in 3-D
  SweepSet lines;              // angles marching along z or y
  int row_slot = -1;           // slot of the angle along x, or -1
  bool skip1 = false;          // two-table walk: runs of length 1 are not recorded, finalize restores them from the x angle's runs
  bool fused = false;          // one [prev][len][cur] table instead of separate GLCM / GLRLM tables
  int LPL = 1;                 // lines per lane of the lines kernel (1, 2, 4)
  int pitch = 0, padw = 0;     // row pitch / periodic pad of the packed level volume
  bool vec_rows = false;       // Nx multiple of 16: vector pack and vector row staging
  AngleSet aset;               // all angles embedded in 3-D (for multi_check_kernel)
  // lines kernel configuration
  int RS = 0;                  // GLRLM run lengths kept in LDS (>= Nr: every length, no long-run path)
  bool LONG = false;
  int threads = 256;
  size_t lds_bytes = 0;
  // rows kernel configuration (512 threads, 8 staging tiles behind the histograms)
  int RSr = 0;
  bool LONGr = false;
  size_t lds_bytes_rows = 0;
  // fixed-window lines kernel (kernels_sweepfw.h): rows of 65..1024 voxels, fused table
  bool fw = false;
  int fwK = 8;                 // window columns per lane (4: rows up to 256, 8: up to 512, 16: up to 1024)
  int fw_blocks = 1;           // workgroups of the line roles
  int fw_threads = 1024;       // threads per workgroup of the fixed-window launch
  int fw_rows_threads = 512;   // ... and of the x angle's launch (sweep_fw_rows_kernel: one staging tile per wave)
  int RSfw = 0;                // run-length slots of its table (one workgroup per CU: most of the 160 KB)
  bool LONGfw = false;
  size_t lds_fw = 0;
  int RSfw_rows = 0;           // length slots of the rows role's table (it shares the LDS with 16 staging tiles)
  size_t lds_fw_rows = 0;      // the x angle as a launch of its own (sweep_fw_rows_kernel)
  int fw_xblocks = 0;          // > 0: the x angle is the trailing role of the fixed-window launch, this many workgroups behind fw_blocks
  // two-table fixed-window kernel (kernels_sweepfw2.h): 40 .. 170 grey levels
  bool fw2 = false;
  int RS2 = 0;                 // run-length slots per level row
  int fw2_copies = 1;          // copies of the run-length slots in a row (lane l uses copy l mod copies)
  bool LONGfw2 = false;
  size_t lds_fw2 = 0;
  int pitch16 = 0;             // bytes per row of the 16-bit level volume
  // the x angle of a two-table volume on the 16-bit levels (sweep_fw2_rows_kernel): table + one staging tile per wave
  bool fw2_rows = false;
  int RS2r = 0, fw2r_copies = 1, fw2r_waves = 16;
  bool LONGfw2r = false;
  size_t lds_fw2_rows = 0;
  FwSet fwset;
};

// what the planner is asked: a call's shape (not its data)
struct PlanInput {
  int nd = 0;
  const int *size = nullptr;     // [nd]
  const int *angles = nullptr;   // host [Na][nd]
  int Na = 0;
  int Ng = 0, Nr = 0;
  bool want_glcm = false, want_glrlm = false;
  bool voxel_mode = false;       // a voxel list: never a sweep
};

constexpr size_t kHistBudget = 72 * 1024;      // LDS bytes a lines workgroup may spend on histograms
constexpr size_t kHistBudgetRows = 36 * 1024;  // same for a rows workgroup (which also holds staging tiles)
constexpr int kRowsThreads = 512;
constexpr size_t kHistBudgetFw = 146 * 1024;   // fixed-window kernel: one 16-wave workgroup per CU (+ its dead zone)

// largest RS (<= Nr) whose table fits `budget` bytes; -1 if not even RS = 1 fits
inline int fit_rs(bool glcm, bool glrlm, bool fused, int Ng, int Nr, size_t budget) {
  int lo = 0, hi = Nr;
  if (sizeof(u32) * (size_t)hist_layout(glcm, glrlm, fused, Ng, 1).words > budget) return -1;
  lo = 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (sizeof(u32) * (size_t)hist_layout(glcm, glrlm, fused, Ng, mid).words <= budget) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// LDS bank of a bin of the fused table = (row stride * prev + len + cur) mod 32 with row stride = (RS+1)(Ng+1) words.  On
// smooth images cur ~ prev +- 1, so the banks of one ds_add spread like (stride+1) * prev: give up a few length slots (at most
// 12, never below 16) for a stride whose (stride+1) is odd and 5..11 banks away from 0 (512^3 smooth levels: 0.74 ms at
// stride = 0 mod 32, 0.57 ms at 22).  A table that holds every length (rs >= Nr) stays as it is.
inline int bank_stride_rs(int rs, int Ng, int Nr) {
  if (rs >= Nr) return rs;
  for (int r = rs; r >= std::max(16, rs - 12); r--) {
    const int d = (((r + 1) * (Ng + 1)) % 32 + 1) % 32, dist = std::min(d, 32 - d);
    if ((d & 1) && dist >= 5 && dist <= 11) return r;
  }
  return rs;
}

// Table choice: the fused [prev][len][cur] table, the two tables of the fixed-window kernel for 40+ levels, or separate GLCM /
// GLRLM tables -- and the shape of the lines and rows kernels of kernels_sweep.h that follows from it.  false: no table fits.
inline bool plan_tables(SweepPlan &p, const PlanInput &in, const SweepKnobs &kn, int Nr) {
  const int Ng = in.Ng;
  const bool want_glcm = in.want_glcm, want_glrlm = in.want_glrlm;
  // fused table when both matrices are wanted and it holds run lengths up to at least min(Nr, 8)
  if (want_glcm && want_glrlm) {
    const int rs = fit_rs(true, true, true, Ng, Nr, kHistBudget);
    const int rsr = fit_rs(true, true, true, Ng, Nr, kHistBudgetRows);
    if (Ng <= (255 >> PRAD_FUSED_SHIFT) && rs >= std::min(Nr, 8) && rsr >= std::min(Nr, 4)) {
      p.fused = true;
      p.RS = rs;
      p.RSr = rsr;
    }
  }
  // Two-table fixed-window kernel for the line angles when the fused table does not fit (40+ levels): rows that one wave
  // window covers, a level row [Ng + 1 pairs | RS2 lengths] table within the LDS, and the rows kernel (separate tables, here
  // with up to 100 KB for them) for the angle along x
  if (want_glcm && want_glrlm && !p.fused && Ng >= 40 && p.Nx > 64 && p.Nx <= 512 && !kn.no_fw2) {
    // run-length slots per level row and copies of them (lane l adds to copy l mod C): as many copies as leave >= 32 slots
    // (or every length), slots capped at 64 -- longer runs take the checked path, and empty slots cost zeroing and flushing
    const long long maxwords = (158 * 1024) / 4;
    const long long room = maxwords / (Ng + 1) - (Ng + 1);
    int copies = 1;
    long long rs2 = std::min<long long>(room, Nr);
    for (int cc = 8; cc >= 2; cc >>= 1)
      if (room / cc >= std::min<long long>(32, Nr)) {
        copies = cc;
        rs2 = std::min<long long>(std::min<long long>(room / cc, 64), Nr);
        break;
      }
    if (kn.fw2_copies.set) {   // tuning override
      copies = std::max(1, std::min(8, (int)kn.fw2_copies.v));
      rs2 = std::min<long long>(std::min<long long>(room / copies, copies > 1 ? 64 : Nr), Nr);
    }
    if (kn.fw2_rs.set) rs2 = std::min<long long>(rs2, kn.fw2_rs.v);   // tuning override
    if (rs2 < Nr && ((Ng + 1 + copies * rs2) & 1) == 0) rs2--;      // odd row stride: consecutive levels on different banks
    const int rsr = fit_rs(true, true, false, Ng, Nr, 116 * 1024);   // (+ 40 KB of staging tiles: within the 160 KB)
    if ((rs2 >= 24 || rs2 >= Nr) && rs2 >= 1 && rsr >= std::min(Nr, 4)) {
      p.fw2 = true;
      p.skip1 = !kn.fw2_noskip1;   // (needs the x angle in the call: cleared when it is not)
      p.RS2 = (int)rs2;
      p.LONGfw2 = rs2 < Nr;
      p.fw2_copies = copies;
      p.lds_fw2 = 4 * fw2_table_words(Ng, p.RS2, copies);
      p.RS = 0;
      p.RSr = rsr;
      // the x angle with the same two tables: as many waves (16, 8, 4 -- the walk is a serial chain per lane) as leave the
      // table next to their 5 KB staging tiles >= 32 length slots (4 waves: >= 24); else the rows kernel of kernels_sweep.h on
      // the 8-bit copy
      for (int waves = 16; waves >= 4 && !p.fw2_rows && !kn.no_fw2_rows; waves >>= 1) {
        if (kn.fw2_rows_waves.set && (int)kn.fw2_rows_waves.v != waves) continue;   // tuning override
        const long long mw = ((158 * 1024) - (long long)waves * 64 * PRAD_ROW16_PITCH) / 4;
        const long long rm = mw / (Ng + 1) - (Ng + 1);
        if (rm < std::min<long long>(waves > 4 ? 32 : 24, Nr)) continue;
        int cc = 1;
        long long r2 = std::min<long long>(std::min<long long>(rm, 64), Nr);
        for (int c2 = 4; c2 >= 2; c2 >>= 1)
          if (rm / c2 >= std::min<long long>(32, Nr)) {
            cc = c2;
            r2 = std::min<long long>(std::min<long long>(rm / c2, 64), Nr);
            break;
          }
        if (r2 < Nr && ((Ng + 1 + cc * r2) & 1) == 0) r2--;      // odd row stride, as above
        if (r2 < 1) continue;
        p.fw2_rows = true;
        p.RS2r = (int)r2;
        p.fw2r_copies = cc;
        p.fw2r_waves = waves;
        p.LONGfw2r = r2 < Nr;
        p.lds_fw2_rows = ((4 * fw2_table_words(Ng, p.RS2r, cc) + 15) & ~(size_t)15) + (size_t)waves * 64 * PRAD_ROW16_PITCH;
      }
    }
  }
  if (!p.fused && !p.fw2) {
    p.RS = want_glrlm ? fit_rs(want_glcm, true, false, Ng, Nr, kHistBudget) : 0;
    p.RSr = want_glrlm ? fit_rs(want_glcm, true, false, Ng, Nr, kHistBudgetRows) : 0;
    if (p.RS < 0 || p.RSr < 0) return false;
    if (!want_glrlm && sizeof(u32) * (size_t)hist_layout(true, false, false, Ng, 0).words > kHistBudgetRows) return false;
  }
  p.LONG = want_glrlm && p.RS < Nr;
  p.LONGr = want_glrlm && p.RSr < Nr;
  p.lds_bytes = sizeof(u32) * (size_t)hist_layout(want_glcm, want_glrlm, p.fused, Ng, p.RS).words;
  p.threads = p.lds_bytes <= 20 * 1024 ? 256 : (p.lds_bytes <= 40 * 1024 ? 512 : 1024);
  if (kn.threads.set) {  // tuning/ablation override
    const int v = (int)kn.threads.v;
    if (v == 256 || v == 512 || v == 1024) p.threads = v;
  }
  const size_t hw = (size_t)hist_layout(want_glcm, want_glrlm, p.fused, Ng, p.RSr).words;
  p.lds_bytes_rows = sizeof(u32) * ((hw + 3) & ~(size_t)3) + (kRowsThreads / 64) * 64 * PRAD_ROW_PITCH;
  return true;
}

// The packed level volume and the lines kernel's shape.  Each lane of the lines kernel owns LPL adjacent lines; rows get a
// periodic pad of one wave width unless a fixed-window kernel (which masks instead of wrapping) walks them.
inline void plan_lines_shape(SweepPlan &p, const PlanInput &in, const SweepKnobs &kn, int cus) {
  // Lines per lane: more lines amortise the per-step overhead (a chunk of 256 / 128 / 64 lines costs about
  // 1.0 / 0.575 / 0.33 per step), fewer lines waste less of a partial last chunk and give the dynamic hand-out more,
  // smaller chunks.  Estimate the walk time of one angle as (chunks per wave + half a chunk of tail) x chunk cost.
  {
    const double waves = std::max(1.0, (double)(cus / std::max(1, std::min(in.Na, 12))) * 16.0);
    const double cost[3] = {1.0, 0.575, 0.33};
    const int cand[3] = {4, 2, 1};
    double best = 1e300;
    p.LPL = 1;
    for (int i = 0; i < 3; i++) {
      if (cand[i] > 1 && p.Nx < 48 * cand[i]) continue;        // lanes would mostly idle
      const double chunks = (double)std::max(p.Ny, 1) * ((p.Nx + 64 * cand[i] - 1) / (64 * cand[i]));
      const double t = (chunks <= waves ? 1.0 : chunks / waves + 0.5) * cost[i];
      if (t < best) {
        best = t;
        p.LPL = cand[i];
      }
    }
  }
  if (kn.lpl.set) {  // tuning/ablation override
    const int v = (int)kn.lpl.v;
    if (v == 1 || v == 2 || v == 4) p.LPL = v;
  }
  p.vec_rows = (p.Nx % 16) == 0;
  // fixed-window kernel: needs the fused table and rows that one wave window (64 lanes x 4, 8 or 16 columns) covers
  p.fw = p.fused && p.Nx > 64 && p.Nx <= 1024 && !kn.no_fw;
  p.fwK = p.Nx <= 256 ? 4 : (p.Nx <= 512 ? 8 : 16);
  if (p.fw2) p.fwK = p.Nx <= 256 ? 4 : 8;
  p.padw = (p.fw || p.fw2) ? 0 : std::min(64 * p.LPL, p.Nx);
  p.pitch16 = 2 * ((p.Nx + 7) & ~7);
  p.pitch = (p.Nx + p.padw + 15) & ~15;   // 16-byte aligned rows: vector staging in the rows kernel for any Nx
}

// The angle list split into line roles (angles that march along z or y) and the x slot.  false: not a list for the sweeps
// (an offset beyond +-1, a first moving component that is not +1 as in a unidirectional list, two x angles).
inline bool plan_angles(SweepPlan &p, const PlanInput &in) {
  p.lines.count = 0;
  p.aset.count = in.Na;
  for (int a = 0; a < in.Na; a++) {
    int o[3] = {0, 0, 0};
    for (int d = 0; d < in.nd; d++) o[3 - in.nd + d] = in.angles[a * in.nd + d];
    int first = 0;
    for (int d = 0; d < 3; d++) {
      if (o[d] < -1 || o[d] > 1) return false;
      if (!first && o[d]) first = o[d];
      p.aset.off[a][d] = o[d];
    }
    if (first != 1) return false;  // sweeps assume the first moving component is +1 (unidirectional list)
    if (o[0] == 0 && o[1] == 0) {
      if (p.row_slot >= 0) return false;
      p.row_slot = a;
      continue;
    }
    SweepDesc &D = p.lines.d[p.lines.count++];
    D.slot = a;
    D.NX = p.Nx;
    D.dx = o[2];
    if (o[0] == 1) {  // march z, rows = y
      D.NM = p.Nz; D.NU = p.Ny; D.du = o[1];
      D.sM = (long long)p.Ny * p.pitch; D.sU = p.pitch;
    } else {          // march y, rows = z (never moves)
      D.NM = p.Ny; D.NU = p.Nz; D.du = 0;
      D.sM = p.pitch; D.sU = (long long)p.Ny * p.pitch;
    }
    D.LXc = (p.Nx + 64 * p.LPL - 1) / (64 * p.LPL);
    D.chunks = (long long)D.NU * D.LXc;
  }
  return true;
}

// The fixed-window launch: its table, the x angle's launch, and the workgroups of every line role.
inline void plan_fw_launch(SweepPlan &p, const PlanInput &in, const SweepKnobs &kn, int Nr, int cus) {
  const int Ng = in.Ng;
  size_t budget = kHistBudgetFw;
  if (kn.fw_budget_kb.set) budget = (size_t)std::max(8, (int)kn.fw_budget_kb.v) * 1024;   // tuning override
  p.RSfw = bank_stride_rs(fit_rs(true, true, true, Ng, Nr, budget), Ng, Nr);
  if (kn.fw_rs.set) p.RSfw = std::max(1, std::min(p.RSfw, (int)kn.fw_rs.v));   // tuning override
  p.LONGfw = p.RSfw < Nr;
  p.lds_fw = fw_lds_bytes(hist_layout(true, true, true, Ng, p.RSfw));
  if (p.row_slot >= 0 && p.fw) {   // the x angle: a launch of its own, 8 waves + their staging tiles (sweep_fw_rows_kernel)
    if (kn.fw_rows_threads.set) p.fw_rows_threads = std::max(64, std::min(1024, (int)kn.fw_rows_threads.v & ~63));   // tuning override
    const size_t tiles = (size_t)(p.fw_rows_threads / 64) * 64 * PRAD_ROW_PITCH;
    p.RSfw_rows = bank_stride_rs(fit_rs(true, true, true, Ng, Nr, std::min<size_t>(100 * 1024, (size_t)160 * 1024 - 2048 - tiles)), Ng, Nr);
    p.lds_fw_rows = ((fw_lds_bytes(hist_layout(true, true, true, Ng, p.RSfw_rows)) + 15) & ~(size_t)15) + tiles;
  }
  // Roles of the one launch (kernels_sweepfw.h sweep_fw_kernel): one per line angle, one 16-wave workgroup per CU over
  // all of them (1-D grid)
  const int nroles = p.lines.count;
  int total = cus;
  if (kn.fw_blocks.set) total = std::max(nroles, (int)kn.fw_blocks.v);   // tuning override: workgroups of the launch
  if (kn.fw_threads.set) p.fw_threads = std::max(64, std::min(1024, (int)kn.fw_threads.v & ~63));   // ... and their size
  // The remainder of the division goes to the roles that cost most per line: the wave life by role of
  // profiles/r05_fw_phases.md x the workgroups each role had gives 19.5 - 19.6 (lines that drift in x AND wrap in the row
  // dimension), 18.8 - 19.2 (one of the two), 18.1 - 18.5 (neither)
  int bonus[PRAD_MAX_SWEEP] = {0};
  {
    int left = total % nroles;
    for (int cls = 2; cls >= 0 && left > 0; cls--)
      for (int r = 0; r < nroles && left > 0; r++) {
        const SweepDesc &S = p.lines.d[r];
        const int c = (S.dx != 0 ? 1 : 0) + (S.du != 0 ? 1 : 0);
        if (c == cls && !bonus[r]) {
          bonus[r] = 1;
          left--;
        }
      }
  }
  p.fwset.first_block[0] = 0;
  for (int r = 0; r < nroles; r++) p.fwset.first_block[r + 1] = p.fwset.first_block[r] + total / nroles + bonus[r];
  for (int r = nroles + 1; r < PRAD_MAX_SWEEP + 1; r++) p.fwset.first_block[r] = p.fwset.first_block[nroles];
  p.fw_blocks = p.fwset.first_block[nroles];
}

// The x angle of a fused-table GLCM + GLRLM call: trailing workgroups of the same launch (kernels_sweepfw.h sweep_fw_kernel),
// as many as its own launch would have, shaped like that launch's (fw_rows_threads / 64 walking waves, one staging tile each,
// behind a table of RSfw_rows length slots).  PRAD_FW_XROLE=0: the two launches.
inline void plan_fw_xrole(SweepPlan &p, const SweepKnobs &kn, int cus) {
  p.fwset.xslot = -1;
  p.fwset.xRS = 0;
  p.fwset.xwaves = 0;
  p.fwset.xgpd = 1;
  if (!(p.fw && p.fused && p.row_slot >= 0 && p.fw_threads == 1024 && !kn.fw_xrole_off)) return;
  const long long groups = fw_row_groups((long long)p.Nz * p.Ny);
  const int wpb = p.fw_rows_threads / 64;
  long long xb = std::min<long long>((groups + wpb - 1) / wpb, (long long)cus);
  if (kn.fw_xblocks.set) xb = std::min<long long>(kn.fw_xblocks.v, 4096);   // tuning override
  p.fw_xblocks = (int)std::max<long long>(1, xb);
  p.fwset.first_block[p.lines.count + 1] = p.fw_blocks + p.fw_xblocks;
  p.fwset.xslot = p.row_slot;
  p.fwset.xRS = p.RSfw_rows;
  p.fwset.xwaves = wpb;
  p.fwset.xgpd = 1;   // (groups per pull: more only coarsens the hand-out, see fw_rows_role)
  if (kn.fw_xgpd.set) p.fwset.xgpd = std::max(1, std::min(64, (int)kn.fw_xgpd.v));   // tuning override
}

// Piece lengths: every line role's march is cut into pieces so that each of its waves finds about per_wave chunks.
// false: more chunks than an int counts (cannot happen below 2^31 voxels).
inline bool plan_fw_pieces(SweepPlan &p, const SweepKnobs &kn) {
  int per_wave = 6;
  if (kn.fw_per_wave.set) per_wave = std::max(1, (int)kn.fw_per_wave.v);
  p.fwset.count = p.lines.count;
  p.fwset.NX = p.Nx;
  // XCD-aware chunk hand-out (kernels_sweepfw.h): opt-in -- it takes the fabric reads of the level volume from 10.2 to 3.9
  // per volume at 512^3 but its 8 shorter pieces cost 4 % of time (profiles/r03_probes.md), and time is the metric
  p.fwset.xcd = 0;
  if (kn.fw_xcd.set) p.fwset.xcd = ((p.fw || p.fw2) && p.Nz >= 64 && kn.fw_xcd.v != 0) ? 1 : 0;
  for (int i = 0; i < p.lines.count; i++) {
    const SweepDesc &S = p.lines.d[i];
    FwDesc &D = p.fwset.d[i];
    D.slot = S.slot; D.NM = S.NM; D.NU = S.NU; D.du = S.du; D.dx = S.dx; D.sM = S.sM; D.sU = S.sU;
    p.fwset.pitch = p.pitch;
    if (p.fw2) {   // byte strides of the 16-bit level volume
      const bool march_z = S.sM >= S.sU;
      D.sM = march_z ? (long long)p.Ny * p.pitch16 : p.pitch16;
      D.sU = march_z ? p.pitch16 : (long long)p.Ny * p.pitch16;
      p.fwset.pitch = p.pitch16;
    }
    p.fwset.nrows = p.Nz * p.Ny;
    const long long want = (long long)per_wave * (p.fwset.first_block[i + 1] - p.fwset.first_block[i]) * (p.fw_threads / 64);
    int pieces = (int)std::max<long long>(1, (want + D.NU - 1) / D.NU);
    int CL = ((D.NM + pieces - 1) / pieces + 7) & ~7;
    CL = std::max(CL, D.NM >= 128 ? 64 : 16);   // (shorter pieces only multiply the piece start / tail overhead)
    const bool march_z_role = S.sM >= S.sU && p.Nz > 1;
    D.dom_kind = march_z_role ? 0 : 1;
    if (p.fwset.xcd && march_z_role) CL = std::max(32, ((D.NM + PRAD_FW_DOMAINS - 1) / PRAD_FW_DOMAINS + 7) & ~7);   // a piece = an XCD's z-slab
    if (kn.fw_cl.set) CL = std::max(8, (int)kn.fw_cl.v & ~7);
    D.CL = CL;
    D.pieces = (D.NM + CL - 1) / CL;
    const long long chunks = (long long)D.NU * D.pieces;
    if (chunks > 2000000000LL) return false;
    D.chunks = (int)chunks;
  }
  return true;
}

// Can this call run on the sweep kernels, and how?  (p.ok = false: the pairs tier or the exact kernels take it.)  Segment mode,
// Nd <= 3, unit angles of a unidirectional list, up to 255 grey levels, Nr at least the longest edge.
inline SweepPlan plan_sweep(const PlanInput &in, const SweepKnobs &kn, int cus) {
  SweepPlan p;
  if (in.voxel_mode || in.nd > 3 || in.Ng < 1 || in.Ng > 255 || in.Na > PRAD_MAX_SWEEP) return p;
  int dims[3] = {1, 1, 1};
  for (int d = 0; d < in.nd; d++) dims[3 - in.nd + d] = in.size[d];
  p.Nz = dims[0]; p.Ny = dims[1]; p.Nx = dims[2];
  const int longest = std::max(dims[0], std::max(dims[1], dims[2]));
  if (in.want_glrlm && in.Nr < longest) return p;  // a run could overflow Nr
  const int Nr = in.want_glrlm ? in.Nr : 1;
  if (!plan_tables(p, in, kn, Nr)) return p;
  plan_lines_shape(p, in, kn, cus);
  if (!plan_angles(p, in)) return p;
  if ((p.fw || p.fw2) && p.lines.count > 0) {
    plan_fw_launch(p, in, kn, Nr, cus);
    plan_fw_xrole(p, kn, cus);
    if (!plan_fw_pieces(p, kn)) return p;   // -> generic path
  } else {
    p.fw = false;
    if (p.fw2) return SweepPlan();   // (only the x angle was asked for: not worth a plan of its own) -> generic path
  }
  if (p.row_slot < 0) p.skip1 = false;   // no x angle in this call: nothing to restore the runs of length 1 from
  p.ok = true;
  return p;
}

#pragma GCC visibility pop
}  // namespace prad
