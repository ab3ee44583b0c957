// prad_api.hip -- C ABI (include/pyradiomics_amd.h) of the MI355X texture-matrix engine.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC prad_api.hip -o libpyradiomics_amd.so
//
// Dispatch policy (per call):
//   segment mode, Nd <= 3, unit angles, Ng small enough for LDS-private histograms
//       -> pack_levels + sweep kernels (kernels_sweep.h)            path "sweep"
//   anything else (voxel mode, Nd > 3, |offset| > 1, large Ng), or a volume whose masked levels fall outside
//   [1, Ng] (detected on the device by pack_levels)
//       -> exact generic kernels (kernels_generic.h)                 path "generic"
// GLDM / NGTDM: byte kernels (kernels_neigh.h, path "neigh"), then the 16-bit tier (kernels_pairs.h, path "pairs": planned by
// prad_neigh_plan.h, executed by pairs_neigh below), then the exact kernels.
// There is no host-side compute path: without a HIP device every calculate_* call fails with PRAD_E_HIP.
#include "prad_runtime.h"
#include "kernels_generic.h"
#include "kernels_pairs.h"
#include "kernels_sweep.h"
#include "kernels_sweepfw.h"
#include "kernels_sweepfw2.h"
#include "kernels_neigh.h"
#include "kernels_voxel.h"
#include "kernels_voxslide.h"
#include "kernels_mcc.h"
#include "kernels_voxtex.h"
#include "prad_sweep_plan.h"
#include "prad_pipe_plan.h"
#include "prad_neigh_plan.h"
#include "prad_internal.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <limits>
#include <mutex>
#include <thread>

using namespace prad;

namespace {
const char *kVersion = "pyradiomics_amd 0.1.0 (gfx950)";
}  // namespace

namespace prad {   // (prad_internal.h: prad_image.hip enumerates the angles of an image too)
// ------------------------------------------------------------------------------------------------
// angle enumeration (cmatrices.c:756-892), host side: tiny, integer, runs once per call
// ------------------------------------------------------------------------------------------------
int angle_count(const int *size, const int *distances, int Nd, int Ndist, int bidirectional, int f2d) {
  long long total = 0;
  for (int k = 0; k < Ndist; k++) {
    const int dist = distances[k];
    if (dist < 1) return 0;
    long long shell_outer = 1, shell_inner = 1;
    for (int d = 0; d < Nd; d++) {
      if (d == f2d) continue;
      if (dist < size[d]) {
        shell_outer *= 2LL * dist + 1;
        shell_inner *= 2LL * dist - 1;
      } else {
        const long long reach = 2LL * (size[d] - 1) + 1;
        shell_outer *= reach;
        shell_inner *= reach;
      }
    }
    total += shell_outer - shell_inner;
  }
  if (!bidirectional) total /= 2;
  return (int)total;
}

int angle_build(const int *size, const int *distances, int Nd, int Ndist, int f2d, int Na, int *angles) {
  int maxd = 0;
  for (int k = 0; k < Ndist; k++) {
    if (distances[k] < 1) return 1;
    maxd = std::max(maxd, distances[k]);
  }
  // enumerate offset vectors in the reference's order: every component runs +maxd .. -maxd, last
  // dimension fastest (cmatrices.c:843-860); emit the legal ones whose infinity norm was requested.
  std::vector<int> off(Nd, maxd);
  int got = 0;
  long long guard = 1;
  for (int d = 0; d < Nd; d++) guard *= (2LL * maxd + 1);
  for (long long it = 0; it < guard && got < Na; it++) {
    int norm = 0;
    bool legal = true;
    for (int d = 0; d < Nd && legal; d++) {
      const int o = off[d];
      if ((d == f2d && o != 0) || o >= size[d] || o <= -size[d]) legal = false;
      norm = std::max(norm, std::abs(o));
    }
    if (legal && norm >= 1) {
      for (int k = 0; k < Ndist; k++)
        if (distances[k] == norm) {
          std::copy(off.begin(), off.end(), angles + (size_t)got * Nd);
          got++;
          break;
        }
    }
    for (int d = Nd - 1; d >= 0; d--) {
      if (off[d] > -maxd) { off[d]--; break; }
      off[d] = maxd;
    }
  }
  return got == Na ? 0 : 1;
}
static_assert(kMaxSweepAngles == PRAD_MAX_SWEEP, "prad_internal.h: kMaxSweepAngles");
static_assert(kPairMaxAngles == PRAD_PAIR_MAXA && sizeof(PairsNeighPlan().o) == sizeof(PairAngles().o) && kPairLdsBytes == PRAD_PAIR_LDS_WORDS * 4,
              "prad_neigh_plan.h: the kernels' table sizes");
}  // namespace prad

namespace {

// ------------------------------------------------------------------------------------------------
// call setup shared by all matrices
// ------------------------------------------------------------------------------------------------
struct Call {
  Context *c;
  hipStream_t s;
  Geo g;
  VoxMode vm;
  const int32_t *image;   // device
  const uint8_t *mask;    // device
  const int *angles_h;    // host [Na][Nd]
  int *angles_d;          // device copy
  int Na;
  int *flags_d;           // device int[4]: [0] pack saw irregular level, [1] generic index error, [2] sweep LDS base != 0, [3] the pack kernel saw a voxel outside the ROI
  int *flags_h;           // pinned
};

int setup_call(Call &k, const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
               int Na, int Nvox, const int *voxels_dev, int kernelRadius, int force2Ddim, hipStream_t s,
               bool zero_flags = true) {
  Context &c = ctx();
  k.c = &c;
  k.s = s;
  if (!image || !mask) return fail(PRAD_E_ARG, "image/mask is NULL");
  if (!angles || Na < 1) return fail(PRAD_E_ARG, "angles is NULL or Na < 1");
  PRAD_TRY(make_geo(size, Nd, &k.g));
  if (Nvox < 1) return fail(PRAD_E_ARG, "Nvox=%d < 1", Nvox);
  k.vm.nvox = Nvox;
  k.vm.voxels = voxels_dev;
  k.vm.radius = kernelRadius;
  k.vm.f2d = force2Ddim;
  if (voxels_dev) {
    if (kernelRadius <= 0) return fail(PRAD_E_ARG, "Expecting kernelRadius > 0");  // _cmatrices.c:1091-1095
    long long b = 1;
    for (int d = 0; d < Nd; d++)
      if (d != force2Ddim) b *= std::min<long long>(2LL * kernelRadius + 1, k.g.size[d]);
    k.vm.boxmax = b;
  } else {
    if (Nvox != 1) return fail(PRAD_E_ARG, "Nvox=%d without a voxel list", Nvox);
    k.vm.boxmax = k.g.n;
  }
  k.image = image;
  k.mask = mask;
  k.angles_h = angles;
  k.Na = Na;
  {
    int *prev = nullptr;
    auto it = c.bufs.find(c.key("angles"));
    if (it != c.bufs.end()) prev = (int *)it->second.p;
    PRAD_TRY(c.get<int>("angles", (size_t)Na * Nd, &k.angles_d));
    std::vector<int> &cached = c.angle_cache();
    const bool same = prev == k.angles_d && cached.size() == (size_t)Na * Nd &&
                      std::equal(cached.begin(), cached.end(), angles);
    if (!same) {   // (a copy from pageable memory blocks the host: skip it when the table on the device is current)
      PRAD_HIP(hipMemcpyAsync(k.angles_d, angles, sizeof(int) * Na * Nd, hipMemcpyHostToDevice, s));
      PRAD_HIP(hipStreamSynchronize(s));
      cached.assign(angles, angles + (size_t)Na * Nd);
    }
  }
  PRAD_TRY(c.get<int>("flags", 4, &k.flags_d));
  if (zero_flags) PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));   // (the sweep path zeroes them with its accumulators)
  void *fh = nullptr;
  PRAD_TRY(c.get_pinned("flags_h", sizeof(int) * 4, &fh));
  k.flags_h = (int *)fh;
  return PRAD_OK;
}

int read_flags(Call &k) {
  PRAD_HIP(hipMemcpyAsync(k.flags_h, k.flags_d, sizeof(int) * 4, hipMemcpyDeviceToHost, k.s));
  PRAD_HIP(hipStreamSynchronize(k.s));
  return PRAD_OK;
}

inline unsigned blocks_for(long long threads, int bs = 256) { return (unsigned)((threads + bs - 1) / bs); }

int check_grid(long long threads, const char *what) {
  if ((threads + 255) / 256 > 2147483647LL)
    return fail(PRAD_E_UNSUPPORTED, "%s: %lld work items exceed the launch grid; split the voxel batch", what, threads);
  return PRAD_OK;
}

// ------------------------------------------------------------------------------------------------
// generic launches
// ------------------------------------------------------------------------------------------------
int generic_glcm(Call &k, int Ng, double *out) {
  const size_t per = (size_t)Ng * Ng * k.Na;
  PRAD_HIP(hipMemsetAsync(out, 0, sizeof(double) * per * k.vm.nvox, k.s));
  const long long threads = (long long)k.vm.nvox * k.vm.boxmax;
  PRAD_TRY(check_grid(threads, "GLCM"));
  Timed t(*k.c, "generic", k.s);
  hipLaunchKernelGGL(gen_glcm_kernel, dim3(blocks_for(threads)), dim3(256), 0, k.s, k.g, k.vm, k.image, k.mask,
                     k.angles_d, k.Na, Ng, out, k.flags_d + 1);
  return check_launch("gen_glcm_kernel");
}

int generic_glrlm(Call &k, int Ng, int Nr, double *out) {
  const size_t per = (size_t)Ng * Nr * k.Na;
  PRAD_HIP(hipMemsetAsync(out, 0, sizeof(double) * per * k.vm.nvox, k.s));
  int *multi = nullptr;
  PRAD_TRY(k.c->get<int>("multi", (size_t)k.vm.nvox * k.Na, &multi));
  PRAD_HIP(hipMemsetAsync(multi, 0, sizeof(int) * k.vm.nvox * k.Na, k.s));
  const long long threads = (long long)k.vm.nvox * k.vm.boxmax * k.Na;
  PRAD_TRY(check_grid(threads, "GLRLM"));
  Timed t(*k.c, "generic", k.s);
  hipLaunchKernelGGL(gen_glrlm_kernel, dim3(blocks_for(threads)), dim3(256), 0, k.s, k.g, k.vm, k.image, k.mask,
                     k.angles_d, k.Na, Ng, Nr, out, multi, k.flags_d + 1);
  PRAD_TRY(check_launch("gen_glrlm_kernel"));
  const long long pthreads = (long long)k.vm.nvox * Ng * k.Na;
  hipLaunchKernelGGL(glrlm_prune_kernel, dim3(blocks_for(pthreads)), dim3(256), 0, k.s, out, multi, k.vm.nvox, Ng,
                     Nr, k.Na);
  return check_launch("glrlm_prune_kernel");
}

int generic_gldm(Call &k, int Ng, int alpha, double *out) {
  const size_t per = (size_t)Ng * (2 * (size_t)k.Na + 1);
  PRAD_HIP(hipMemsetAsync(out, 0, sizeof(double) * per * k.vm.nvox, k.s));
  const long long threads = (long long)k.vm.nvox * k.vm.boxmax;
  PRAD_TRY(check_grid(threads, "GLDM"));
  Timed t(*k.c, "generic", k.s);
  hipLaunchKernelGGL(gen_gldm_kernel, dim3(blocks_for(threads)), dim3(256), 0, k.s, k.g, k.vm, k.image, k.mask,
                     k.angles_d, k.Na, Ng, alpha, out, k.flags_d + 1);
  return check_launch("gen_gldm_kernel");
}

int generic_ngtdm(Call &k, int Ng, double *out) {
  Timed t(*k.c, "generic", k.s);
  if (k.vm.voxels) {
    hipLaunchKernelGGL(gen_ngtdm_voxel_kernel, dim3(blocks_for(k.vm.nvox, 64)), dim3(64), 0, k.s, k.g, k.vm,
                       k.image, k.mask, k.angles_d, k.Na, Ng, out, k.flags_d + 1);
    return check_launch("gen_ngtdm_voxel_kernel");
  }
  unsigned long long *acc = nullptr;
  const size_t nacc = (size_t)Ng * (k.Na + 1);
  PRAD_TRY(k.c->get<unsigned long long>("ngtdm_acc", nacc, &acc));
  PRAD_HIP(hipMemsetAsync(acc, 0, sizeof(unsigned long long) * nacc, k.s));
  PRAD_TRY(check_grid(k.g.n, "NGTDM"));
  hipLaunchKernelGGL(gen_ngtdm_segment_kernel, dim3(blocks_for(k.g.n)), dim3(256), 0, k.s, k.g, k.vm, k.image,
                     k.mask, k.angles_d, k.Na, Ng, acc, k.flags_d + 1);
  PRAD_TRY(check_launch("gen_ngtdm_segment_kernel"));
  hipLaunchKernelGGL(ngtdm_finalize_kernel, dim3(blocks_for(Ng, 64)), dim3(64), 0, k.s, acc, Ng, k.Na, out);
  return check_launch("ngtdm_finalize_kernel");
}

// ------------------------------------------------------------------------------------------------
// sweep path (segment mode GLCM / GLRLM)
// ------------------------------------------------------------------------------------------------
int cu_count() {
  static thread_local int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
  }
  return cus;
}

// The switches of the GLCM / GLRLM route (prad_sweep_plan.h SweepKnobs) are an argument `kn` of everything below that depends on
// one.  Every GLCM / GLRLM call (texture_pairs_runs) and every other entry point that finds a volume to flush (join, mark,
// status, ...: pipeline_flush(c)) reads the environment afresh -- once -- and passes the record down, so that a test can flip a
// checker switch (PRAD_FIN_RIDE, PRAD_FINALIZE_ONE, PRAD_FW_XROLE, ...) inside one process.
SweepPlan plan_sweep(const Call &k, const SweepKnobs &kn, int Ng, int Nr, bool want_glcm, bool want_glrlm) {
  PlanInput in;
  in.nd = k.g.nd;
  in.size = k.g.size;
  in.angles = k.angles_h;
  in.Na = k.Na;
  in.Ng = Ng;
  in.Nr = Nr;
  in.want_glcm = want_glcm;
  in.want_glrlm = want_glrlm;
  in.voxel_mode = k.vm.voxels != nullptr;
  return plan_sweep(in, kn, cu_count());
}

template <bool G, bool R, bool LNG, bool F, int LPL>
int launch_lines_lpl(Call &k, const SweepKnobs &kn, const SweepPlan &p, const uint8_t *levels, int Ng, int Nr, u32 *glcm_acc,
                     u32 *glrlm_acc, int *multi) {
  long long maxchunks = 0;
  for (int i = 0; i < p.lines.count; i++) maxchunks = std::max(maxchunks, p.lines.d[i].chunks);
  const int wpb = p.threads / 64;
  // Chunks (one NM-step serial walk of 64*LPL lines) are grabbed dynamically.  ONE workgroup per CU across all angles
  // measured best at 512^3 (20-21 workgroups per angle on 256 CUs: 0.64 ms; 42, i.e. two per CU: 0.66 ms; anything
  // between makes some CUs host two workgroups while others host one: 0.75-0.93 ms): with ~3 chunks per wave the
  // tail is short, and a lone workgroup has the CU's LDS bandwidth to itself.
  const long long blocks_avail = std::max<long long>(1, (long long)cu_count() / p.lines.count);
  unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(blocks_avail, (maxchunks + wpb - 1) / wpb));
  if (kn.lines_blocks.set && kn.lines_blocks.v >= 1) gx = (unsigned)kn.lines_blocks.v;  // tuning override: workgroups per angle
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_lines_kernel<G, R, LNG, F, LPL>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
  hipLaunchKernelGGL((sweep_lines_kernel<G, R, LNG, F, LPL>), dim3(gx, p.lines.count), dim3(p.threads), p.lds_bytes,
                     k.s, p.lines, levels, Ng, Nr, p.RS, glcm_acc, glrlm_acc, multi, multi + PRAD_MAX_SWEEP,
                     k.flags_d);
  return check_launch("sweep_lines_kernel");
}

template <bool G, bool R, bool LNG, bool F>
int launch_lines(Call &k, const SweepKnobs &kn, const SweepPlan &p, const uint8_t *levels, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
                 int *multi) {
  if (p.LPL == 4) return launch_lines_lpl<G, R, LNG, F, 4>(k, kn, p, levels, Ng, Nr, glcm_acc, glrlm_acc, multi);
  if (p.LPL == 2) return launch_lines_lpl<G, R, LNG, F, 2>(k, kn, p, levels, Ng, Nr, glcm_acc, glrlm_acc, multi);
  return launch_lines_lpl<G, R, LNG, F, 1>(k, kn, p, levels, Ng, Nr, glcm_acc, glrlm_acc, multi);
}

template <bool LNG, int K, bool HASPAD, bool PACK>
int launch_fw_kpp(Call &k, const SweepPlan &p, const PackJob &pj, const FinJob &fj, const uint8_t *levels, const uint8_t *rowzero, int Ng, int Nr,
                  u32 *glcm_acc, u32 *glrlm_acc, int *multi, int *flags_d) {
  // one block size and one LDS size per grid: the x angle's trailing workgroups (table + staging tiles) may need more than the walk's
  const size_t lds = p.fw_xblocks > 0 ? std::max(p.lds_fw, p.lds_fw_rows) : p.lds_fw;
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_fw_kernel<LNG, K, HASPAD, PACK>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((sweep_fw_kernel<LNG, K, HASPAD, PACK>), dim3(p.fw_blocks + p.fw_xblocks), dim3(p.fw_threads), lds, k.s, p.fwset, pj, fj,
                     levels, rowzero, Ng, Nr, p.RSfw, glcm_acc, glrlm_acc, multi + 2 * PRAD_MAX_SWEEP + PRAD_FW_WORK_STRIDE, flags_d);
  return check_launch("sweep_fw_kernel");
}
template <bool LNG, int K, bool HASPAD>
int launch_fw_kp(Call &k, const SweepPlan &p, const PackJob &pj, const FinJob &fj, const uint8_t *levels, const uint8_t *rowzero, int Ng, int Nr,
                 u32 *glcm_acc, u32 *glrlm_acc, int *multi, int *flags_d) {
  if (pj.n16 > 0) return launch_fw_kpp<LNG, K, HASPAD, true>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
  return launch_fw_kpp<LNG, K, HASPAD, false>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
}
template <bool LNG, int K>
int launch_fw_k(Call &k, const SweepPlan &p, const PackJob &pj, const FinJob &fj, const uint8_t *levels, const uint8_t *rowzero, int Ng, int Nr,
                u32 *glcm_acc, u32 *glrlm_acc, int *multi, int *flags_d) {
  if (p.Nx != 64 * K) return launch_fw_kp<LNG, K, true>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
  return launch_fw_kp<LNG, K, false>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
}
// the fixed-window launch of one volume: every line angle and, optionally, the pack of the NEXT volume as a side job; with a pack,
// `fj` may carry the finalize of the volume BEFORE and the zeroing for the next ones (FinJob)
int launch_fw(Call &k, const SweepPlan &p, const PackJob &pj, const FinJob &fj, const uint8_t *levels, const uint8_t *rowzero, int Ng, int Nr,
              u32 *glcm_acc, u32 *glrlm_acc, int *multi, int *flags_d) {
  if (p.fwK == 16)   // rows of 513 .. 1024 voxels: 16 columns per lane
    return p.LONGfw ? launch_fw_k<true, 16>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d)
                    : launch_fw_k<false, 16>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
  if (p.LONGfw) return p.fwK == 4 ? launch_fw_k<true, 4>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d)
                                : launch_fw_k<true, 8>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
  return p.fwK == 4 ? launch_fw_k<false, 4>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d)
                    : launch_fw_k<false, 8>(k, p, pj, fj, levels, rowzero, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
}

template <bool LNG, int K, bool HASPAD, bool SKIP1, bool PACK>
int launch_fw2_khsp(Call &k, const SweepPlan &p, const PackJob &pj, const uint8_t *levels16, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
                    int *work, int *flags_d) {
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_fw2_kernel<LNG, K, HASPAD, SKIP1, PACK>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_fw2));
  hipLaunchKernelGGL((sweep_fw2_kernel<LNG, K, HASPAD, SKIP1, PACK>), dim3(p.fw_blocks), dim3(1024), p.lds_fw2, k.s, p.fwset, pj, levels16,
                     Ng, Nr, p.RS2, p.fw2_copies, glcm_acc, glrlm_acc, work, flags_d);
  return check_launch("sweep_fw2_kernel");
}
template <bool LNG, int K, bool HASPAD, bool SKIP1>
int launch_fw2_khs(Call &k, const SweepPlan &p, const PackJob &pj, const uint8_t *levels16, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
                   int *work, int *flags_d) {
  if (pj.n16 > 0) return launch_fw2_khsp<LNG, K, HASPAD, SKIP1, true>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d);
  return launch_fw2_khsp<LNG, K, HASPAD, SKIP1, false>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d);
}
template <bool LNG, int K>
int launch_fw2_k(Call &k, const SweepPlan &p, const PackJob &pj, const uint8_t *levels16, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
                 int *multi, int *flags_d) {
  int *work = multi + 2 * PRAD_MAX_SWEEP + PRAD_FW_WORK_STRIDE;
  if (p.Nx != 64 * K)
    return p.skip1 ? launch_fw2_khs<LNG, K, true, true>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d)
                   : launch_fw2_khs<LNG, K, true, false>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d);
  return p.skip1 ? launch_fw2_khs<LNG, K, false, true>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d)
                 : launch_fw2_khs<LNG, K, false, false>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, work, flags_d);
}
// the two-table launch of one volume: every line angle and, optionally, the pack of the NEXT volume as a side job
int launch_fw2(Call &k, const SweepPlan &p, const PackJob &pj, const uint8_t *levels16, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
               int *multi, int *flags_d) {
  if (p.LONGfw2) return p.fwK == 4 ? launch_fw2_k<true, 4>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d)
                                 : launch_fw2_k<true, 8>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
  return p.fwK == 4 ? launch_fw2_k<false, 4>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d)
                    : launch_fw2_k<false, 8>(k, p, pj, levels16, Ng, Nr, glcm_acc, glrlm_acc, multi, flags_d);
}

template <bool LNG>
int launch_fw_rows(Call &k, const SweepPlan &p, const uint8_t *levels, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc, int *flags_d) {
  const long long nrows = (long long)p.Nz * p.Ny, groups = fw_row_groups(nrows);
  const int wpb = p.fw_rows_threads / 64;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((groups + wpb - 1) / wpb, (long long)cu_count()));
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_fw_rows_kernel<LNG>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_fw_rows));
  hipLaunchKernelGGL((sweep_fw_rows_kernel<LNG>), dim3(gx), dim3(p.fw_rows_threads), p.lds_fw_rows, k.s, levels, nrows, p.Nx,
                     p.pitch, p.row_slot, Ng, Nr, p.RSfw_rows, glcm_acc, glrlm_acc, flags_d);
  return check_launch("sweep_fw_rows_kernel");
}

template <bool LNG>
int launch_fw2_rows(Call &k, const SweepPlan &p, const uint8_t *levels16, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc, int *flags_d) {
  const long long nrows = (long long)p.Nz * p.Ny, groups = nrows >= 4096 ? ((nrows + 511) / 512) * 8 : (nrows + 63) / 64;
  const int wpb = p.fw2r_waves;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((groups + wpb - 1) / wpb, (long long)cu_count()));
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_fw2_rows_kernel<LNG>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_fw2_rows));
  hipLaunchKernelGGL((sweep_fw2_rows_kernel<LNG>), dim3(gx), dim3(64 * wpb), p.lds_fw2_rows, k.s, levels16, nrows, p.Nx, p.pitch16,
                     p.row_slot, Ng, Nr, p.RS2r, p.fw2r_copies, glcm_acc, glrlm_acc, flags_d);
  return check_launch("sweep_fw2_rows_kernel");
}

template <bool G, bool R, bool LNG, bool F>
int launch_rows(Call &k, const SweepPlan &p, const uint8_t *levels, int Ng, int Nr, u32 *glcm_acc, u32 *glrlm_acc,
                int *multi) {
  const long long nrows = (long long)p.Nz * p.Ny;
  const long long groups = (nrows + 63) / 64;
  const int wpb = kRowsThreads / 64;
  const int per_cu = std::max(1, std::min(2048 / kRowsThreads, (int)(160 * 1024 / p.lds_bytes_rows)));
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((groups + wpb - 1) / wpb, (long long)cu_count() * per_cu));
  PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&sweep_rows_kernel<G, R, LNG, F>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes_rows));
  hipLaunchKernelGGL((sweep_rows_kernel<G, R, LNG, F>), dim3(gx), dim3(kRowsThreads), p.lds_bytes_rows, k.s, levels,
                     nrows, p.Nx, p.pitch, p.row_slot, Ng, Nr, p.RSr, glcm_acc, glrlm_acc, multi, k.flags_d);
  return check_launch("sweep_rows_kernel");
}

// zeroes three word ranges in one launch (a: 16-byte aligned, any length)
__global__ void __launch_bounds__(256) zero3_kernel(u32 *__restrict__ a, size_t na, u32 *__restrict__ b, size_t nb,
                                                    u32 *__restrict__ c3, size_t nc) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  uint4 *a4 = reinterpret_cast<uint4 *>(a);
  for (size_t i = t; i < na / 4; i += nt) a4[i] = make_uint4(0, 0, 0, 0);
  for (size_t i = (na & ~(size_t)3) + t; i < na; i += nt) a[i] = 0;
  for (size_t i = t; i < nb; i += nt) b[i] = 0;
  for (size_t i = t; i < nc; i += nt) c3[i] = 0;
}

#include "prad_pipeline.h"   // VolState, ZeroNeed, launch_zero3 and the deferred pipeline

// workspace of a volume (the set Context::lane) and, in z, what must be zero before its pack and its sweeps
int vol_prepare(Call &k, const SweepPlan &p, int Ng, int Nr, double *glcm, double *glrlm, VolState &v, ZeroNeed &z) {
  Context &c = *k.c;
  v.p = p;
  v.Ng = Ng;
  v.Nr = Nr;
  v.Na = k.Na;
  v.glcm = glcm;
  v.glrlm = glrlm;
  v.flags_d = k.flags_d;
  const long long nrows = (long long)p.Nz * p.Ny;
  // (a two-table volume whose x angle walks the 16-bit elements keeps no byte copy: round 5b)
  v.levels = nullptr;
  if (!(p.fw2 && p.fw2_rows && p.lines.count > 0 && p.row_slot >= 0)) {
    PRAD_TRY(c.get<uint8_t>("levels", (size_t)nrows * p.pitch + 1024, &v.levels));
    v.levels += 512;   // the fixed-window kernel reads (and masks) up to one window before the first and behind the last row
  }
  v.levels16 = nullptr;
  if (p.fw2) {
    PRAD_TRY(c.get<uint8_t>("levels16", (size_t)nrows * p.pitch16 + 4096, &v.levels16));
    v.levels16 += 2048;
  }
  const size_t nglcm = glcm ? (size_t)k.Na * Ng * Ng : 0, nglrlm = glrlm ? (size_t)k.Na * Ng * Nr : 0;
  // accumulators, then per-angle "multi-element" flags, then per-role work counters of the lines kernels
  const size_t nctl = 2 * PRAD_MAX_SWEEP + (size_t)PRAD_FW_WORK_STRIDE * (PRAD_FW_DOMAINS * PRAD_MAX_SWEEP + 1);
  PRAD_TRY(c.get<u32>("sweep_acc", nglcm + nglrlm + nctl, &v.acc));
  v.glcm_acc = v.acc;
  v.glrlm_acc = v.acc + nglcm;
  v.multi = (int *)(v.acc + nglcm + nglrlm);
  v.rowzero = nullptr;
  if (p.fw) PRAD_TRY(c.get<uint8_t>("rowzero", (size_t)nrows + 64, &v.rowzero));
  // accumulators + control words, row flags and the volume's flag words start from zero
  z.p[kZeroAcc] = v.acc;
  z.w[kZeroAcc] = nglcm + nglrlm + nctl;
  z.p[kZeroRz] = reinterpret_cast<u32 *>(v.rowzero);
  z.w[kZeroRz] = v.rowzero ? ((size_t)nrows + 3) / 4 : 0;
  z.p[kZeroFl] = reinterpret_cast<u32 *>(v.flags_d);
  z.w[kZeroFl] = kFlagWords;
  return PRAD_OK;
}

int vol_pack_standalone(Call &k, VolState &v) {
  Context &c = *k.c;
  const SweepPlan &p = v.p;
  Timed t(c, "pack", k.s);
  if (p.fw2) {   // 16-bit elements for the line walks + plain 8-bit levels for the rows kernel, one pass
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n / 4 + 255) / 256, 8192));
    hipLaunchKernelGGL(pack_levels16_kernel, dim3(gx), dim3(256), 0, k.s, k.image, k.mask, k.g.n, p.Nx, p.pitch16, p.pitch, v.Ng,
                       v.levels16, v.levels, v.flags_d);
    return check_launch("pack_levels16_kernel");
  }
  const int vec_ok = p.vec_rows && ((((uintptr_t)k.image) | ((uintptr_t)k.mask) | ((uintptr_t)v.levels)) & 15) == 0;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n / 16 + 255) / 256, 4096));
  // the fused walker reads level*4 bytes (see Walker<true, true, LONG, true>); the planner takes it for Ng <= 36
  const int shift = (v.glcm && v.glrlm && p.fused) ? PRAD_FUSED_SHIFT : 0;
  hipLaunchKernelGGL(pack_levels_kernel, dim3(gx), dim3(256), 0, k.s, k.image, k.mask, k.g.n, p.Nx, p.pitch, p.padw,
                     v.Ng, v.levels, v.flags_d, vec_ok, shift, v.rowzero);
  return check_launch("pack_levels_kernel");
}

template <bool G, bool R, bool F>
int launch_sweeps(Call &k, const SweepKnobs &kn, const VolState &v, const PackJob &pj, const FinJob &fj) {
  const SweepPlan &p = v.p;
  if (p.lines.count > 0 && p.fw && G && R && F) {
    {
      Timed t(*k.c, "sweep", k.s);
      PRAD_TRY(launch_fw(k, p, pj, fj, v.levels, v.rowzero, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi, v.flags_d));
    }
    if (p.row_slot >= 0 && p.fw_xblocks == 0) {   // (else the x angle ran as the trailing role of that launch)
      Timed t(*k.c, "rows", k.s);
      if (p.RSfw_rows < v.Nr) PRAD_TRY(launch_fw_rows<true>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.flags_d));
      else PRAD_TRY(launch_fw_rows<false>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.flags_d));
    }
    return PRAD_OK;
  }
  if (p.fw2 && G && R && !F && p.lines.count > 0) {
    {
      Timed t(*k.c, "sweep", k.s);
      PRAD_TRY(launch_fw2(k, p, pj, v.levels16, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi, v.flags_d));
    }
    if (p.row_slot >= 0) {
      Timed t(*k.c, "rows", k.s);
      if (p.fw2_rows) {
        if (p.LONGfw2r) PRAD_TRY(launch_fw2_rows<true>(k, p, v.levels16, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.flags_d));
        else PRAD_TRY(launch_fw2_rows<false>(k, p, v.levels16, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.flags_d));
      } else if (p.LONGr) {
        PRAD_TRY((launch_rows<G, R, true, F>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
      } else {
        PRAD_TRY((launch_rows<G, R, false, F>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
      }
    }
    return PRAD_OK;
  }
  Timed t(*k.c, "sweep", k.s);
  if (p.lines.count > 0) {
    if (R && p.LONG) PRAD_TRY((launch_lines<G, R, true, F>(k, kn, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
    else PRAD_TRY((launch_lines<G, R, false, F>(k, kn, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
  }
  if (p.row_slot >= 0) {
    if (R && p.LONGr) PRAD_TRY((launch_rows<G, R, true, F>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
    else PRAD_TRY((launch_rows<G, R, false, F>(k, p, v.levels, v.Ng, v.Nr, v.glcm_acc, v.glrlm_acc, v.multi)));
  }
  return PRAD_OK;
}

// the sweeps of volume v; `pj` (n16 > 0) = the pack of another volume as a side job of the fixed-window launch
int vol_sweep(Call &k, const SweepKnobs &kn, const VolState &v, const PackJob &pj, const FinJob &fj) {
  if (pj.n16 > 0 && !pipeline_volume(v.p, v.glcm != nullptr, v.glrlm != nullptr))
    return fail(PRAD_E_ARG, "internal: a pack job needs a fixed-window host launch");
  if (pj.n16 > 0 && (pj.levels16 != nullptr) != v.p.fw2)
    return fail(PRAD_E_ARG, "internal: the pack job's layout is not the host launch's");
  if (!fin_job_empty(fj) && !(v.glcm && v.glrlm && v.p.fused && v.p.fw && v.p.lines.count > 0))
    return fail(PRAD_E_ARG, "internal: a finalize job needs a fused-table host launch");
  if (v.glcm && v.glrlm && v.p.fused) return launch_sweeps<true, true, true>(k, kn, v, pj, fj);
  if (v.glcm && v.glrlm) return launch_sweeps<true, true, false>(k, kn, v, pj, fj);
  if (v.glcm) return launch_sweeps<true, false, false>(k, kn, v, pj, fj);
  return launch_sweeps<false, true, false>(k, kn, v, pj, fj);
}
int vol_sweep(Call &k, const SweepKnobs &kn, const VolState &v, const PackJob &pj) {
  FinJob none;
  memset(&none, 0, sizeof(none));
  return vol_sweep(k, kn, v, pj, none);
}

__global__ void latch_flags_kernel(const int *__restrict__ flags, int *__restrict__ sticky) {
  if (flags[0] || flags[2]) sticky[0] = 1;
}

// deferred GLDM / NGTDM calls: any flag (levels outside [1, Ng] under the mask, a declined fast path) is a verdict to latch
__global__ void latch_any_flag_kernel(const int *__restrict__ flags, int *__restrict__ sticky) {
  if (flags[0] || flags[1] || flags[2]) sticky[0] = 1;
}
int latch_neigh(Context &c, Call &k) {
  int *sticky = nullptr;
  PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
  hipLaunchKernelGGL(latch_any_flag_kernel, dim3(1), dim3(1), 0, k.s, (const int *)k.flags_d, sticky);
  return check_launch("latch_any_flag_kernel");
}

// u32 accumulators -> float64 matrices in the reference layouts; `sticky` (deferred calls): latch the levels verdict
int vol_finalize(Call &k, const SweepKnobs &kn, const VolState &v, int *sticky) {
  Context &c = *k.c;
  const SweepPlan &p = v.p;
  const int Ng = v.Ng, Nr = v.Nr, Na = v.Na;
  double *glcm = v.glcm, *glrlm = v.glrlm;
  bool latched = false;
  {
    Timed t(c, "finalize", k.s);
    const bool runs_diag = p.fused || p.fw2;     // the walks left the GLCM diagonal to the runs
    // SKIP1 walks (fw2) did not count their runs of length 1: only finalize_glcm_diag_kernel puts them back, and it needs both
    // matrices and the x angle's complete run table (plans with skip1 always carry them: plan_sweep clears the flag otherwise)
    if (p.fw2 && p.skip1 && p.lines.count > 0 && !(glcm && glrlm && p.row_slot >= 0))
      return fail(PRAD_E_UNSUPPORTED, "sweep plan derives runs of length 1 but the call cannot restore them");
    if (glcm && glrlm && runs_diag && kn.finalize_one && (long long)Ng * Nr < (1LL << 30)) {
      // ONE launch (finalize_volume_kernel): Na angle workgroups, then the two element-wise conversions
      const int nbR = (int)blocks_for((long long)Ng * Nr * Na, 1024), nbG = (int)blocks_for((long long)Ng * Ng * Na, 1024);
      const int restore_from = (p.fw2 && p.skip1 && p.lines.count > 0) ? p.row_slot : -1;
      if (v.levels)
        hipLaunchKernelGGL(finalize_volume_kernel<uint8_t>, dim3(Na + nbR + nbG), dim3(1024), 0, k.s, p.aset, (const uint8_t *)v.levels,
                           p.Nz, p.Ny, p.Nx, p.pitch, v.glcm_acc, v.glrlm_acc, Ng, Nr, Na, nbR, glcm, glrlm, v.multi,
                           restore_from, (const int *)v.flags_d, sticky);
      else
        hipLaunchKernelGGL(finalize_volume_kernel<unsigned short>, dim3(Na + nbR + nbG), dim3(1024), 0, k.s, p.aset,
                           reinterpret_cast<const unsigned short *>(v.levels16), p.Nz, p.Ny, p.Nx, p.pitch16 / 2, v.glcm_acc,
                           v.glrlm_acc, Ng, Nr, Na, nbR, glcm, glrlm, v.multi, restore_from, (const int *)v.flags_d, sticky);
      PRAD_TRY(check_launch("finalize_volume_kernel"));
      latched = sticky != nullptr;
      glcm = glrlm = nullptr;   // both matrices are complete
    }
    if (glcm && glrlm && runs_diag) {
      const int nb1 = (int)blocks_for((long long)Ng * Ng * Na), nb2 = (Ng * Na + 3) / 4;
      hipLaunchKernelGGL(finalize_glcm_diag_kernel, dim3(nb1 + nb2), dim3(256), 0, k.s, v.glcm_acc, v.glrlm_acc, Ng, Nr, Na, nb1,
                         glcm, v.multi, (p.fw2 && p.skip1 && p.lines.count > 0) ? p.row_slot : -1);
      PRAD_TRY(check_launch("finalize_glcm_diag_kernel"));
    } else if (glcm) {
      hipLaunchKernelGGL(finalize_glcm_kernel, dim3(blocks_for((long long)Ng * Ng * Na)), dim3(256), 0, k.s,
                         v.glcm_acc, v.glrlm_acc, Ng, Nr, Na, p.fused ? 1 : 0, glcm);
      PRAD_TRY(check_launch("finalize_glcm_kernel"));
    }
    if (glrlm && runs_diag) {
      if (!glcm) {
        hipLaunchKernelGGL(glcm_diag_resolve_kernel, dim3(Ng, Na), dim3(64), 0, k.s, v.glcm_acc, v.glrlm_acc, Ng, Nr, Na,
                           glcm, v.multi);
        PRAD_TRY(check_launch("glcm_diag_resolve_kernel"));
      }
      if (v.levels)
        hipLaunchKernelGGL(multi_check_kernel<uint8_t>, dim3(128, Na), dim3(256), 0, k.s, p.aset, (const uint8_t *)v.levels, p.Nz, p.Ny,
                           p.Nx, p.pitch, v.multi);
      else
        hipLaunchKernelGGL(multi_check_kernel<unsigned short>, dim3(128, Na), dim3(256), 0, k.s, p.aset,
                           reinterpret_cast<const unsigned short *>(v.levels16), p.Nz, p.Ny, p.Nx, p.pitch16 / 2, v.multi);
      PRAD_TRY(check_launch("multi_check_kernel"));
    }
    if (glrlm) {
      hipLaunchKernelGGL(finalize_glrlm_kernel, dim3(blocks_for((long long)Ng * Nr * Na)), dim3(256), 0, k.s,
                         v.glrlm_acc, v.multi, Ng, Nr, Na, glrlm, (const int *)v.flags_d, sticky);
      PRAD_TRY(check_launch("finalize_glrlm_kernel"));
      latched = sticky != nullptr;
    }
  }
  if (sticky && !latched) {
    hipLaunchKernelGGL(latch_flags_kernel, dim3(1), dim3(1), 0, k.s, v.flags_d, sticky);
    PRAD_TRY(check_launch("latch_flags_kernel"));
  }
  return PRAD_OK;
}

// returns PRAD_OK with *used=false if the device found irregular levels (caller then runs generic)
int sweep_glcm_glrlm(Call &k, const SweepKnobs &kn, const SweepPlan &p, int Ng, int Nr, double *glcm, double *glrlm, bool *used) {
  Context &c = *k.c;
  VolState v;
  ZeroNeed z;
  PRAD_TRY(vol_prepare(k, p, Ng, Nr, glcm, glrlm, v, z));
  PRAD_TRY(launch_zero3(k.s, z));
  PRAD_TRY(vol_pack_standalone(k, v));
  PackJob pj;
  memset(&pj, 0, sizeof(pj));
  PRAD_TRY(vol_sweep(k, kn, v, pj));
  int *sticky = nullptr;       // deferred calls latch their levels verdict
  if (c.deferred) PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
  PRAD_TRY(vol_finalize(k, kn, v, sticky));
  if (c.deferred) {   // enqueue only: the verdict on the levels is latched for prad_deferred_status()
    *used = true;
    return PRAD_OK;
  }
  PRAD_TRY(read_flags(k));
  // flags[2]: the fused walker found its table away from LDS address 0 and did nothing (cannot happen with the current
  // toolchain: the dynamic array is the kernels' only LDS object) -- let the generic kernels redo the call
  *used = (k.flags_h[0] == 0 && k.flags_h[2] == 0);
  return PRAD_OK;
}

// the 16-bit level volume of the pairs tier (GLCM / GLRLM below, GLDM / NGTDM in pairs_neigh); flags_d[0]: a level outside 1..Ng
int pairs_pack(Call &k, int Ng, lev16 *L) {
  Timed t(*k.c, "pack", k.s);
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n + 255) / 256, (long long)cu_count() * 16));
  hipLaunchKernelGGL(pairs_pack_kernel, dim3(gx), dim3(256), 0, k.s, k.image, k.mask, k.g.n, Ng, L, k.flags_d);
  return check_launch("pairs_pack_kernel");
}

// GLCM and/or GLRLM, device pointers
// The tier between the sweeps and the exact kernels (kernels_pairs.h): segment mode, Nd <= 3, any offset list of up to 128
// angles, up to 38 400 grey levels.  *used = false when the call is not for it or the pack found a level outside 1..Ng
// (the outputs are then untouched zeros and the exact kernels redo the call).
int pairs_glcm_glrlm(Call &k, const SweepKnobs &kn, int Ng, int Nr, double *glcm, double *glrlm, bool *used) {
  *used = false;
  Context &c = *k.c;
  if (k.vm.voxels || k.g.nd > 3 || Ng < 1 || Ng > PRAD_PAIR_LDS_WORDS || k.Na > PRAD_PAIR_MAXA || k.g.n >= 0x7fffffffLL ||
      kn.no_pairs)
    return PRAD_OK;
  int dims[3] = {1, 1, 1};
  for (int d = 0; d < k.g.nd; d++) dims[3 - k.g.nd + d] = k.g.size[d];
  PairAngles A;
  memset(&A, 0, sizeof(A));
  A.n = k.Na;
  for (int a = 0; a < k.Na; a++)
    for (int d = 0; d < k.g.nd; d++) {
      const int o = k.angles_h[a * k.g.nd + d];
      if (o < -127 || o > 127) return PRAD_OK;
      A.o[a][3 - k.g.nd + d] = (signed char)o;
    }
  if (glrlm && Nr < std::max(dims[0], std::max(dims[1], dims[2]))) return PRAD_OK;   // a run could overflow Nr: the exact kernels say what the reference says
  const size_t gwords = glcm ? (size_t)k.Na * Ng * Ng : 0, rwords = glrlm ? (size_t)k.Na * Ng * Nr : 0;
  if ((gwords + rwords) * sizeof(u32) > ((size_t)1 << 30)) return PRAD_OK;
  hipStream_t s = k.s;
  lev16 *L = nullptr;
  u32 *gacc = nullptr, *racc = nullptr, *counts = nullptr;
  int *multi = nullptr;
  PRAD_TRY(c.get<lev16>("pairs_levels", (size_t)k.g.n + 8, &L));
  if (glcm) PRAD_TRY(c.get<u32>("pairs_glcm_acc", gwords, &gacc));
  if (glrlm) {
    PRAD_TRY(c.get<u32>("pairs_glrlm_acc", rwords, &racc));
    PRAD_TRY(c.get<u32>("pairs_counts", (size_t)Ng, &counts));
    PRAD_TRY(c.get<int>("pairs_multi", (size_t)PRAD_PAIR_MAXA, &multi));
  }
  PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));
  const int cus = cu_count();
  PRAD_TRY(pairs_pack(k, Ng, L));
  if (glcm) {
    Timed t(c, "pairs", s);
    PRAD_HIP(hipMemsetAsync(gacc, 0, sizeof(u32) * gwords, s));
    int AG, RT, ntile;
    if ((long long)Ng * Ng <= PRAD_PAIR_LDS_WORDS) {
      AG = std::max(1, std::min(k.Na, PRAD_PAIR_LDS_WORDS / (Ng * Ng)));
      RT = Ng;
      ntile = 1;
    } else {
      AG = 1;
      RT = PRAD_PAIR_LDS_WORDS / Ng;
      ntile = (Ng + RT - 1) / RT;
    }
    const int npass = ((k.Na + AG - 1) / AG) * ntile;
    const size_t lds = sizeof(u32) * (size_t)AG * RT * Ng;
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pairs_glcm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // workgroups per pass: the count (2 .. 4 per CU over all passes) that leaves the fewest CUs idle in the last round -- one
    // 150 KB table per CU at a time (186 passes at 300 levels x 3 workgroups were 2.2 rounds, billed as 3)
    long long gbest = 1;
    double ebest = 0;
    for (long long gtry = std::max<long long>(1, 2LL * cus / npass); gtry <= std::max<long long>(1, (4LL * cus + npass - 1) / npass); gtry++) {
      const long long total = gtry * npass, rounds = (total + cus - 1) / cus;
      const double eff = (double)total / (double)(rounds * cus);
      if (eff > ebest + 1e-9) {
        ebest = eff;
        gbest = gtry;
      }
    }
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n / 8 + 1023) / 1024, gbest));
    hipLaunchKernelGGL(pairs_glcm_kernel, dim3(gx, (unsigned)npass), dim3(1024), lds, s, L, dims[0], dims[1], dims[2], A, AG, RT,
                       ntile, Ng, gacc, k.flags_d);
    PRAD_TRY(check_launch("pairs_glcm_kernel"));
    const long long total = (long long)Ng * Ng * k.Na;
    hipLaunchKernelGGL(finalize_glcm_kernel, dim3(blocks_for(total)), dim3(256), 0, s, gacc, (const u32 *)nullptr, Ng, 1, k.Na, 0, glcm);
    PRAD_TRY(check_launch("finalize_glcm_kernel"));
  }
  if (glrlm) {
    Timed t(c, "pairs", s);
    PRAD_HIP(hipMemsetAsync(racc, 0, sizeof(u32) * rwords, s));
    PRAD_HIP(hipMemsetAsync(counts, 0, sizeof(u32) * (size_t)Ng, s));
    PRAD_HIP(hipMemsetAsync(multi, 0, sizeof(int) * PRAD_PAIR_MAXA, s));
    const int use_lds = Ng <= 8192;
    const unsigned gc = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n + 255) / 256, (long long)cus * 8));
    hipLaunchKernelGGL(pairs_level_count_kernel, dim3(gc), dim3(256), use_lds ? sizeof(u32) * (size_t)Ng : 0, s, L, k.g.n, Ng, use_lds,
                       counts, k.flags_d);
    PRAD_TRY(check_launch("pairs_level_count_kernel"));
    const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((k.g.n + 255) / 256, std::max(1LL, 16LL * cus / k.Na)));
    hipLaunchKernelGGL(pairs_glrlm_kernel, dim3(gx, (unsigned)k.Na), dim3(256), 0, s, L, dims[0], dims[1], dims[2], A, Ng, Nr, racc, multi,
                       k.flags_d);
    PRAD_TRY(check_launch("pairs_glrlm_kernel"));
    hipLaunchKernelGGL(pairs_multi_check_kernel, dim3(gx, (unsigned)k.Na), dim3(256), 0, s, A, L, dims[0], dims[1], dims[2], multi, k.flags_d);
    PRAD_TRY(check_launch("pairs_multi_check_kernel"));
    hipLaunchKernelGGL(pairs_run1_kernel, dim3((unsigned)((Ng * k.Na + 3) / 4)), dim3(256), 0, s, racc, counts, Ng, Nr, k.Na, k.flags_d);
    PRAD_TRY(check_launch("pairs_run1_kernel"));
    const long long total = (long long)Ng * Nr * k.Na;
    hipLaunchKernelGGL(finalize_glrlm_kernel, dim3(blocks_for(total)), dim3(256), 0, s, racc, multi, Ng, Nr, k.Na, glrlm,
                       (const int *)nullptr, (int *)nullptr);
    PRAD_TRY(check_launch("finalize_glrlm_kernel"));
  }
  PRAD_TRY(read_flags(k));
  *used = k.flags_h[0] == 0;
  if (!*used) {   // a level outside 1..Ng: leave zeros for the exact kernels (the finalize kernels above wrote only zeros: every
                  // accumulating kernel returned at its first line)
    PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));
  }
  return PRAD_OK;
}

// lanes: a whole-volume deferred call goes onto the next lane -- its stream, which waits for `user`, and a workspace set of its
// own (#0 .. #7 belong to the pipelines' alternating volumes)
int lanes_deal(Context &c, hipStream_t user, hipStream_t *s) {
  c.lane = -1;
  *s = user;
  PRAD_TRY(c.lane_begin(user, s));
  if (c.lane >= 0) c.lane += kAllPipeSets;
  return PRAD_OK;
}

}  // namespace
namespace prad {   // (prad_internal.h)
int texture_pairs_runs(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                       int Na, int Ng, int Nr, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                       double *glcm, double *glrlm, hipStream_t s) {
  if (!glcm && !glrlm) return fail(PRAD_E_ARG, "both outputs are NULL");
  if (Ng < 1 || (glrlm && Nr < 1)) return fail(PRAD_E_ARG, "Ng/Nr must be >= 1");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  const SweepKnobs kn = sweep_knobs_from_env();   // once per call
  struct LaneGuard {
    Context &c;
    ~LaneGuard() { c.lane = -1; }
  } lane_guard{c};
  bool pipe = c.deferred && !voxels && pipeline_mode(kn);
  const hipStream_t user = s;
  int inst = 0;
  if (pipe) PRAD_TRY(pipeline_enter(c, kn, size, Nd, Na, Ng, Nr, glcm, glrlm, &s, &inst));
  else if (c.deferred && !voxels) PRAD_TRY(lanes_deal(c, user, &s));   // lanes mode
  Call k;
  PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, Nvox, voxels, kernelRadius, force2Ddim, s, false));
  SweepPlan p = plan_sweep(k, kn, Ng, Nr, glcm != nullptr, glrlm != nullptr);
  if (pipe && !pipeline_volume(p, glcm != nullptr, glrlm != nullptr)) {
    // Not a volume for the two-stage pipeline (the wrapped-lines kernels): its pack is a launch of its own, so deal the call
    // onto the lanes, where the pack of one volume runs under the walk of the previous one
    PRAD_TRY(pipeline_flush(c, kn));
    PRAD_TRY(pipelines_order(user));   // (twin volumes sit on internal streams: the lane's stream waits for `user`, so for them too)
    pipe = false;
    PRAD_TRY(lanes_deal(c, user, &s));
    PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, Nvox, voxels, kernelRadius, force2Ddim, s, false));
    p = plan_sweep(k, kn, Ng, Nr, glcm != nullptr, glrlm != nullptr);
  }
  PRAD_TRY(c.begin_call(s));
  if (!p.ok) PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));   // (vol_prepare does it on the sweep path)
  bool done = false;
  c.last_variant = !p.ok ? "none" : (p.fw2 ? "fw2" : (p.fw && glcm && glrlm ? "fw" : "lines"));
  if (pipe) {
    PRAD_TRY(pipeline_step(k, kn, inst, p, Ng, Nr, glcm, glrlm));   // (a pipeline volume: the other ones left for the lanes above)
    done = true;
    c.last_path = "sweep";
  }
  if (!done && p.ok) {
    PRAD_TRY(sweep_glcm_glrlm(k, kn, p, Ng, Nr, glcm, glrlm, &done));
    if (done) c.last_path = "sweep";
  }
  if (!done && !c.deferred) {      // (synchronous calls: the tier reads its levels verdict back)
    PRAD_TRY(pairs_glcm_glrlm(k, kn, Ng, Nr, glcm, glrlm, &done));
    if (done) {
      c.last_path = "pairs";
      c.last_variant = "pairs";
    }
  }
  if (!done) {
    if (glcm) PRAD_TRY(generic_glcm(k, Ng, glcm));
    if (glrlm) PRAD_TRY(generic_glrlm(k, Ng, Nr, glrlm));
    PRAD_TRY(read_flags(k));
    c.last_path = "generic";
  }
  PRAD_TRY(c.end_call(s));
  if (c.deferred && done) return PRAD_OK;   // nothing was read back: see prad_deferred_status()
  PRAD_HIP(hipStreamSynchronize(s));
  return k.flags_h[1] ? PRAD_INDEX_ERROR : PRAD_OK;
}
}  // namespace prad
namespace {

// the switches of the GLDM / NGTDM pairs tier, read once per call (DESIGN.md lists them)
NeighKnobs neigh_knobs_from_env() { return {getenv("PRAD_NO_PAIRS") != nullptr, getenv("PRAD_NGTDM_NO_BOX") != nullptr}; }

template <typename WT, int SH>   // the box sums' word: (u32, 24) narrow, (u64, 40)
int launch_pairs_box(Call &k, const PairsNeighPlan &p, const lev16 *L, void *b1, void *b2, int Ng, u64 *acc64) {
  const int *D = p.dims, *flags = k.flags_d;
  hipLaunchKernelGGL((pairs_box_axis_kernel<WT, SH>), dim3(p.box_grid), dim3(256), 0, k.s, L, (const WT *)nullptr, (WT *)b1, D[0],
                     D[1], D[2], 2, p.rad[2], flags);
  hipLaunchKernelGGL((pairs_box_axis_kernel<WT, SH>), dim3(p.box_grid), dim3(256), 0, k.s, (const lev16 *)nullptr, (const WT *)b1,
                     (WT *)b2, D[0], D[1], D[2], 1, p.rad[1], flags);
  auto *kern = p.mode == 2 ? &pairs_ngtdm_box_kernel<2, WT, SH>
             : p.mode == 1 ? &pairs_ngtdm_box_kernel<1, WT, SH> : &pairs_ngtdm_box_kernel<0, WT, SH>;
  if (p.mode) PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.threads), p.lds, k.s, L, (const WT *)b2, D[0], D[1], D[2], p.rad[0], Ng, k.Na + 1,
                     acc64, flags);
  return check_launch("pairs_ngtdm_box_kernel");
}

// GLDM / NGTDM on the 16-bit level volume (kernels_pairs.h): what kernels_neigh.h does not take -- more than 255 levels, bin
// tables beyond its LDS budget.  Whether the tier applies, where the bins live and every launch size: plan_pairs_neigh
// (prad_neigh_plan.h).  Synchronous calls only; *used = false: not for this tier, or a level outside 1..Ng.
int pairs_neigh(Call &k, bool ngtdm, int Ng, int alpha, double *out, bool *used, bool box_only = false) {
  *used = false;
  Context &c = *k.c;
  const PairsNeighInput in = {k.g.nd, k.g.size, k.angles_h, k.Na, Ng, ngtdm, k.vm.voxels != nullptr};
  const PairsNeighPlan p = plan_pairs_neigh(in, neigh_knobs_from_env(), cu_count());
  if (!p.applies || (box_only && !p.box)) return PRAD_OK;
  const size_t bytes = (size_t)Ng * (k.Na + 1) * (ngtdm ? sizeof(u64) : sizeof(u32));
  hipStream_t s = k.s;
  lev16 *L = nullptr;
  void *acc = nullptr;
  PRAD_TRY(c.get<lev16>("pairs_levels", (size_t)k.g.n + 8, &L));
  PRAD_TRY(c.get(ngtdm ? "pairs_ngtdm_acc" : "pairs_gldm_acc", bytes, &acc));
  PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));
  PRAD_TRY(pairs_pack(k, Ng, L));
  {
    Timed t(c, "pairs", s);
    PRAD_HIP(hipMemsetAsync(acc, 0, bytes, s));
    c.last_variant = pairs_variant_name(p.variant);   // which bin placement (and which box-sum word) serves the call
    if (p.box) {
      void *b1 = nullptr, *b2 = nullptr;
      PRAD_TRY(c.get("pairs_box1", (size_t)k.g.n * (p.narrow ? 4 : 8), &b1));
      PRAD_TRY(c.get("pairs_box2", (size_t)k.g.n * (p.narrow ? 4 : 8), &b2));
      if (p.narrow) PRAD_TRY((launch_pairs_box<u32, 24>(k, p, L, b1, b2, Ng, (u64 *)acc)));
      else PRAD_TRY((launch_pairs_box<u64, 40>(k, p, L, b1, b2, Ng, (u64 *)acc)));
    } else {
      PairAngles A;
      A.n = p.na;
      memcpy(A.o, p.o, sizeof(A.o));
      auto *kern = ngtdm ? (p.mode == 2 ? &pairs_neigh_kernel<true, 2> : p.mode == 1 ? &pairs_neigh_kernel<true, 1> : &pairs_neigh_kernel<true, 0>)
                         : (p.mode == 1 ? &pairs_neigh_kernel<false, 1> : &pairs_neigh_kernel<false, 0>);
      if (p.mode) PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
      hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.threads), p.lds, s, A, (const lev16 *)L, p.dims[0], p.dims[1], p.dims[2], Ng, alpha,
                         ngtdm ? nullptr : (u32 *)acc, ngtdm ? (u64 *)acc : nullptr, (const int *)k.flags_d);
      PRAD_TRY(check_launch("pairs_neigh_kernel"));
    }
  }
  if (ngtdm) PRAD_TRY(neigh_finalize_ngtdm(&c, s, (const u64 *)acc, Ng, k.Na, out));
  else PRAD_TRY(neigh_finalize_gldm(&c, s, (const u32 *)acc, Ng, k.Na, out));
  PRAD_TRY(read_flags(k));
  *used = k.flags_h[0] == 0;
  if (!*used) {      // irregular level: the exact kernels redo the call on a zeroed output (the finalize kernels wrote zeros and,
                     // for NGTDM, the level column)
    const size_t outn = ngtdm ? (size_t)Ng * 3 : (size_t)Ng * (2 * k.Na + 1);
    PRAD_HIP(hipMemsetAsync(out, 0, sizeof(double) * outn, s));
    PRAD_HIP(hipMemsetAsync(k.flags_d, 0, sizeof(int) * 4, s));
  }
  return PRAD_OK;
}

int texture_gldm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                 int Ng, int alpha, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, double *out,
                 hipStream_t s) {
  if (!out) return fail(PRAD_E_ARG, "gldm is NULL");
  if (Ng < 1) return fail(PRAD_E_ARG, "Ng must be >= 1");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  Call k;
  PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, Nvox, voxels, kernelRadius, force2Ddim, s));
  PRAD_TRY(c.begin_call(s));
  bool done = false;
  PRAD_TRY(neigh_try_gldm(k.c, k.s, k.g, k.vm, k.image, k.mask, k.angles_h, k.Na, Ng, alpha, out, k.flags_d, &done));
  if (done && c.deferred && !voxels) {   // enqueue only: the flags are latched for prad_deferred_status()
    PRAD_TRY(latch_neigh(c, k));
    c.last_path = "neigh";
    return c.end_call(s);
  }
  bool irregular = false;      // the byte kernels' pack already saw a level outside [1, Ng]: the tier would only find it again
  if (done) {
    PRAD_TRY(read_flags(k));
    done = (k.flags_h[0] == 0);
    irregular = !done;
  }
  if (!done && !c.deferred && !irregular) {
    PRAD_TRY(pairs_neigh(k, false, Ng, alpha, out, &done));
    if (done) c.last_path = "pairs";
  } else if (done) {
    c.last_path = "neigh";
  }
  if (!done) {
    PRAD_TRY(generic_gldm(k, Ng, alpha, out));
    PRAD_TRY(read_flags(k));
    c.last_path = "generic";
    c.last_variant = "none";
  }
  PRAD_TRY(c.end_call(s));
  PRAD_HIP(hipStreamSynchronize(s));
  return k.flags_h[1] ? PRAD_INDEX_ERROR : PRAD_OK;
}

int texture_ngtdm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                  int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, double *out,
                  hipStream_t s) {
  if (!out) return fail(PRAD_E_ARG, "ngtdm is NULL");
  if (Ng < 1) return fail(PRAD_E_ARG, "Ng must be >= 1");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  Call k;
  PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, Nvox, voxels, kernelRadius, force2Ddim, s));
  PRAD_TRY(c.begin_call(s));
  bool done = false;
  if (!c.deferred && !voxels && k.Na > 26) {
    // more neighbours than the 3^3 cube: when they are a whole box (distances [1, 2], [1, 2, 3], ...) the separable box sums of
    // the pairs tier take 0.4 ms per 256^3 volume where the byte kernel visits 124 neighbours per voxel (1.9 ms) and the generic
    // kernels 342 (24 ms)
    PRAD_TRY(pairs_neigh(k, true, Ng, 0, out, &done, true));
    if (done) {
      c.last_path = "pairs";
      PRAD_TRY(c.end_call(s));
      return PRAD_OK;
    }
  }
  PRAD_TRY(neigh_try_ngtdm(k.c, k.s, k.g, k.vm, k.image, k.mask, k.angles_h, k.Na, Ng, out, k.flags_d, &done));
  if (done && c.deferred && !voxels) {   // enqueue only: the flags are latched for prad_deferred_status()
    PRAD_TRY(latch_neigh(c, k));
    c.last_path = "neigh";
    return c.end_call(s);
  }
  bool irregular = false;      // the byte kernels' pack already saw a level outside [1, Ng]: the tier would only find it again
  if (done) {
    PRAD_TRY(read_flags(k));
    done = (k.flags_h[0] == 0);
    irregular = !done;
  }
  if (!done && !c.deferred && !irregular) {
    PRAD_TRY(pairs_neigh(k, true, Ng, 0, out, &done));
    if (done) c.last_path = "pairs";
  } else if (done) {
    c.last_path = "neigh";
  }
  if (!done) {
    PRAD_TRY(generic_ngtdm(k, Ng, out));
    PRAD_TRY(read_flags(k));
    c.last_path = "generic";
    c.last_variant = "none";
  }
  PRAD_TRY(c.end_call(s));
  PRAD_HIP(hipStreamSynchronize(s));
  return k.flags_h[1] ? PRAD_INDEX_ERROR : PRAD_OK;
}

}  // namespace
namespace prad {   // (prad_internal.h)
// GLDM and NGTDM of a segment from one pass over the neighbourhoods (segment mode; prad_calculate_gldm_ngtdm_dev)
int texture_gldm_ngtdm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                       int Ng, int alpha, double *gldm, double *ngtdm, hipStream_t s) {
  if (!gldm || !ngtdm) return fail(PRAD_E_ARG, "gldm / ngtdm is NULL");
  if (Ng < 1) return fail(PRAD_E_ARG, "Ng must be >= 1");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  bool done = false;
  {
    Call k;
    PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, 1, nullptr, 0, -1, s));
    PRAD_TRY(c.begin_call(s));
    PRAD_TRY(neigh_try_both(k.c, k.s, k.g, k.vm, k.image, k.mask, k.angles_h, k.Na, Ng, alpha, gldm, ngtdm, k.flags_d, &done));
    if (done && c.deferred) {   // enqueue only: the flags are latched for prad_deferred_status()
      PRAD_TRY(latch_neigh(c, k));
      c.last_path = "neigh";
      return c.end_call(s);
    }
    if (done) {
      PRAD_TRY(read_flags(k));
      done = (k.flags_h[0] == 0);
      if (done) {
        c.last_path = "neigh";
        PRAD_TRY(c.end_call(s));
        return k.flags_h[1] ? PRAD_INDEX_ERROR : PRAD_OK;
      }
    }
  }
  // not a volume for the packed-byte kernel (or irregular levels: the exact kernels say what the reference says)
  PRAD_TRY(texture_gldm(image, mask, size, Nd, angles, Na, Ng, alpha, 1, nullptr, 0, -1, gldm, s));
  return texture_ngtdm(image, mask, size, Nd, angles, Na, Ng, 1, nullptr, 0, -1, ngtdm, s);
}

// ONE byte-packed copy of a derived image for its neighbourhood pass and its GLSZM (kernels_neigh.h SharedPack), made on `s`
// in front of the image's fork; a buffer per ticket: up to four images are in flight
int image_shared_pack(Context &c, const int32_t *levels, const uint8_t *mask, long long n, int NX, int Ng, int ticket, hipStream_t s) {
  char name[32];
  snprintf(name, sizeof(name), "img_pack%d", ticket);
  uint8_t *pk = nullptr;
  int *pf = nullptr;
  c.workspace = 0;
  PRAD_TRY(c.get<uint8_t>(name, (size_t)n + 64 + 16, &pk));
  pf = (int *)(pk + (((size_t)n + 64 + 3) & ~(size_t)3));
  PRAD_HIP(hipMemsetAsync(pf, 0, sizeof(int) * 2, s));
  const int vec_ok = ((((uintptr_t)levels) | ((uintptr_t)mask) | ((uintptr_t)pk)) & 15) == 0;
  const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>((n / 16 + 255) / 256, 4096));
  hipLaunchKernelGGL(pack_levels_kernel, dim3(gx), dim3(256), 0, s, levels, mask, n, NX, NX, 0, Ng, pk, pf, vec_ok, 0);
  PRAD_TRY(check_launch("pack_levels_kernel"));
  SharedPack &sp = shared_pack();
  sp.image = levels; sp.mask = mask; sp.n = n; sp.Ng = Ng; sp.levels = pk; sp.flags = pf;
  return PRAD_OK;
}
void image_shared_pack_clear() { shared_pack() = SharedPack(); }

int glszm_byte_pack(Context &c, hipStream_t s, const Geo &g, const int32_t *image, const uint8_t *mask, int Ng, int *flags_d,
                    uint8_t **levels) {
  return neigh_pack(&c, s, g, image, mask, Ng, flags_d, levels);
}
}  // namespace prad
namespace {

// z-slab split of one large segment over several GPUs: integer accumulators of a plane range, summed by the
// caller across ranks (RCCL all-reduce of [Ng][Na+1] int64), then finalized once
int neigh_accumulate_i64(int family, const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                         const int *angles, int Na, int Ng, int alpha, int z_lo, int z_hi, long long *acc,
                         hipStream_t s) {
  if (!acc) return fail(PRAD_E_ARG, "acc is NULL");
  if (family != 0 && family != 1) return fail(PRAD_E_ARG, "family must be 0 (GLDM) or 1 (NGTDM)");
  if (Nd != 3) return fail(PRAD_E_UNSUPPORTED, "plane-range accumulators need a 3-D volume (Nd=%d)", Nd);
  if (Ng < 1) return fail(PRAD_E_ARG, "Ng must be >= 1");
  if (z_lo < 0 || z_hi > size[0] || z_lo > z_hi) return fail(PRAD_E_ARG, "plane range [%d, %d) outside 0..%d", z_lo, z_hi, size[0]);
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  Call k;
  PRAD_TRY(setup_call(k, image, mask, size, Nd, angles, Na, 1, nullptr, 0, -1, s));
  PRAD_TRY(c.begin_call(s));
  bool done = false;
  void *raw = nullptr;
  if (family == 0)
    PRAD_TRY(neigh_accumulate<false>(k.c, k.s, k.g, k.vm, k.image, k.mask, k.angles_h, k.Na, Ng, alpha, z_lo, z_hi,
                                     k.flags_d, &raw, &done));
  else
    PRAD_TRY(neigh_accumulate<true>(k.c, k.s, k.g, k.vm, k.image, k.mask, k.angles_h, k.Na, Ng, 0, z_lo, z_hi,
                                    k.flags_d, &raw, &done));
  if (!done) {
    c.end_call(s);
    return fail(PRAD_E_UNSUPPORTED, "plane-range accumulators need Ng <= 255, Na <= %d and [Ng][Na+1] bins within 64 KiB of LDS", PRAD_MAX_NEIGH);
  }
  const long long nacc = (long long)Ng * (Na + 1);
  if (family == 0) {
    hipLaunchKernelGGL(widen_u32_kernel, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, s, (const u32 *)raw, nacc, acc);
    PRAD_TRY(check_launch("widen_u32_kernel"));
  } else {
    PRAD_HIP(hipMemcpyAsync(acc, raw, sizeof(long long) * nacc, hipMemcpyDeviceToDevice, s));
  }
  PRAD_TRY(read_flags(k));
  PRAD_TRY(c.end_call(s));
  PRAD_HIP(hipStreamSynchronize(s));
  // a level outside 1..Ng under the mask: the reference fails the whole calculation (cmatrices.c:744,647)
  return k.flags_h[0] ? PRAD_INDEX_ERROR : PRAD_OK;
}

int neigh_finalize_i64(int family, const long long *acc, int Ng, int Na, double *out, hipStream_t s) {
  if (!acc || !out) return fail(PRAD_E_ARG, "acc/out is NULL");
  if (family != 0 && family != 1) return fail(PRAD_E_ARG, "family must be 0 (GLDM) or 1 (NGTDM)");
  if (Ng < 1 || Na < 1) return fail(PRAD_E_ARG, "Ng and Na must be >= 1");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  PRAD_TRY(c.begin_call(s));
  if (family == 0) {
    const long long nacc = (long long)Ng * (Na + 1);
    u32 *acc32 = nullptr;
    int *flags = nullptr;
    PRAD_TRY(c.get<u32>("gldm_acc", (size_t)nacc, &acc32));
    PRAD_TRY(c.get<int>("flags", 4, &flags));
    PRAD_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 4, s));
    hipLaunchKernelGGL(narrow_i64_kernel, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, s, acc, nacc, acc32, flags);
    PRAD_TRY(check_launch("narrow_i64_kernel"));
    PRAD_TRY(neigh_finalize_gldm(&c, s, acc32, Ng, Na, out));
  } else {
    PRAD_TRY(neigh_finalize_ngtdm(&c, s, reinterpret_cast<const u64 *>(acc), Ng, Na, out));
  }
  PRAD_TRY(c.end_call(s));
  PRAD_HIP(hipStreamSynchronize(s));
  return PRAD_OK;
}

// ------------------------------------------------------------------------------------------------
// host-pointer staging
// ------------------------------------------------------------------------------------------------
struct Staged {
  int32_t *image = nullptr;
  uint8_t *mask = nullptr;
  int *voxels = nullptr;
};

// Large host arrays (the drop-in boundary hands over pageable numpy memory: 671 MB for a 512^3 case) reach the device
// through a ring of pinned buffers: kStageThreads host threads copy 16 MB chunks into the ring while the DMA engine
// drains the chunks already filled.  Measured on the MI355X host (scripts/h2d_bench.hip): 52 GB/s, against 24-28 GB/s for
// hipMemcpyAsync from pageable memory (the runtime's own single-threaded staging) and 17 GB/s for a first-touch
// hipMemcpy (which pins the user's pages on the fly).
constexpr size_t kStageChunk = (size_t)16 << 20;
constexpr int kStageRing = 6;
constexpr int kStageThreads = 4;
constexpr size_t kStageMin = (size_t)32 << 20;   // smaller copies are not worth the thread start-up

struct StageRing {
  char *buf[kStageRing] = {};
  hipEvent_t ev[kStageRing] = {};
  bool busy[kStageRing] = {};
  size_t next = 0;
};
StageRing &stage_ring() {
  static thread_local StageRing r;
  return r;
}

int staged_h2d(Context &c, void *dst, const void *src, size_t bytes, hipStream_t s) {
  if (bytes < kStageMin || getenv("PRAD_NO_STAGING")) {
    PRAD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return PRAD_OK;
  }
  StageRing &r = stage_ring();
  for (int i = 0; i < kStageRing; i++) {
    if (!r.buf[i]) {
      void *p = nullptr;
      PRAD_TRY(c.get_pinned(("stage_ring" + std::to_string(i)).c_str(), kStageChunk, &p));
      r.buf[i] = (char *)p;
      PRAD_HIP(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
    }
  }
  const size_t nchunks = (bytes + kStageChunk - 1) / kStageChunk;
  const size_t first = r.next;
  const bool dbg = getenv("PRAD_STAGE_DEBUG") != nullptr;
  const auto t_begin = std::chrono::steady_clock::now();
  double t_wait_slot = 0, t_wait_copy = 0;
  int nthreads = kStageThreads;
  if (const char *e = getenv("PRAD_STAGE_THREADS")) nthreads = std::max(1, std::min(16, atoi(e)));   // tuning override
  std::atomic<size_t> go{0}, done{0};
  std::atomic<bool> quit{false};
  std::vector<std::thread> workers;
  for (int w = 0; w < nthreads; w++)
    workers.emplace_back([&, w]() {
      size_t seen = 0;
      for (;;) {
        size_t g;
        while ((g = go.load(std::memory_order_acquire)) == seen)
          if (quit.load(std::memory_order_acquire)) return;
        for (size_t ch = seen; ch < g; ch++) {
          const size_t off = ch * kStageChunk, len = std::min(kStageChunk, bytes - off);
          const size_t sl = ((len + nthreads - 1) / nthreads + 63) & ~(size_t)63;
          const size_t a = std::min(len, (size_t)w * sl), b = std::min(len, a + sl);
          if (b > a) memcpy(r.buf[(first + ch) % kStageRing] + a, (const char *)src + off + a, b - a);
          done.fetch_add(1, std::memory_order_release);
        }
        seen = g;
      }
    });
  hipError_t err = hipSuccess;
  for (size_t ch = 0; ch < nchunks && err == hipSuccess; ch++) {
    const int slot = (int)((first + ch) % kStageRing);
    const auto t0 = std::chrono::steady_clock::now();
    if (r.busy[slot]) err = hipEventSynchronize(r.ev[slot]);   // the DMA that last read this slot has finished
    const auto t1 = std::chrono::steady_clock::now();
    go.store(ch + 1, std::memory_order_release);
    while (done.load(std::memory_order_acquire) < (ch + 1) * (size_t)nthreads) {}
    if (dbg) {
      t_wait_slot += std::chrono::duration<double>(t1 - t0).count();
      t_wait_copy += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    }
    const size_t off = ch * kStageChunk, len = std::min(kStageChunk, bytes - off);
    if (err == hipSuccess) err = hipMemcpyAsync((char *)dst + off, r.buf[slot], len, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipEventRecord(r.ev[slot], s);
    r.busy[slot] = true;
  }
  quit.store(true, std::memory_order_release);
  for (auto &t : workers) t.join();
  r.next = (first + nchunks) % kStageRing;
  if (dbg)
    fprintf(stderr, "staged_h2d %zu MB: %.2f ms enqueue (slot waits %.2f ms, host copies %.2f ms)\n", bytes >> 20,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() * 1e3, t_wait_slot * 1e3, t_wait_copy * 1e3);
  if (err != hipSuccess) return fail(PRAD_E_HIP, "staged host-to-device copy failed: %s", hipGetErrorString(err));
  return PRAD_OK;
}

int stage_inputs(Context &c, const int32_t *image, const uint8_t *mask, const int *size, int Nd, int Nvox,
                 const int *voxels, Staged *st) {
  PRAD_TRY(c.ensure_device());
  if (!image || !mask) return fail(PRAD_E_ARG, "image/mask is NULL");
  Geo g;
  PRAD_TRY(make_geo(size, Nd, &g));
  // 16-byte aligned slots so the vectorised pack path applies
  PRAD_TRY(c.get<int32_t>("h_image", (size_t)g.n + 16, &st->image));
  PRAD_TRY(c.get<uint8_t>("h_mask", (size_t)g.n + 64, &st->mask));
  PRAD_TRY(staged_h2d(c, st->image, image, sizeof(int32_t) * g.n, c.own_stream));
  PRAD_TRY(staged_h2d(c, st->mask, mask, g.n, c.own_stream));
  if (voxels) {
    if (Nvox < 1) return fail(PRAD_E_ARG, "Nvox=%d < 1", Nvox);
    PRAD_TRY(c.get<int>("h_voxels", (size_t)Nd * Nvox, &st->voxels));
    PRAD_HIP(hipMemcpyAsync(st->voxels, voxels, sizeof(int) * Nd * Nvox, hipMemcpyHostToDevice, c.own_stream));
  }
  return PRAD_OK;
}

int fetch_output(Context &c, const char *slot, double *host, size_t count, double **dev) {
  (void)host;
  return c.get<double>(slot, count, dev);
}

int copy_back(Context &c, double *host, const double *dev, size_t count) {
  PRAD_HIP(hipMemcpyAsync(host, dev, sizeof(double) * count, hipMemcpyDeviceToHost, c.own_stream));
  PRAD_HIP(hipStreamSynchronize(c.own_stream));
  return PRAD_OK;
}

#include "prad_voxel.h"      // fused voxel-based feature maps

}  // namespace

// =================================================================================================
// extern "C"
// =================================================================================================
extern "C" {

const char *prad_version(void) { return kVersion; }
const char *prad_last_error(void) { return err_state().msg; }
const char *prad_last_path(void) { return ctx().last_path; }
const char *prad_last_variant(void) { return ctx().last_variant; }
#ifdef PRAD_FW_STAMPS
// instrumentation builds only (scripts/r05_fw_stamps.py): per-wave, per-phase cycle sums of the last sweep_fw_kernel launch
// (slot 1: the launch that carries the pack side job, slot 0: the one without)
int prad_debug_fw_stamps(unsigned long long *out, int slot, int nwaves) {
  if (!out || nwaves < 1 || nwaves > 8192 || slot < 0 || slot > 1) return PRAD_E_ARG;
  PRAD_HIP(hipDeviceSynchronize());
  PRAD_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(prad::prad_fw_stamps), sizeof(unsigned long long) * prad::FP_COUNT * (size_t)nwaves,
                               sizeof(unsigned long long) * prad::FP_COUNT * 8192 * (size_t)slot));
  return PRAD_OK;
}
#endif

int prad_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int prad_set_device(int device) {
  int n = prad_device_count();
  if (device < 0 || device >= n) return fail(PRAD_E_ARG, "device %d not in [0,%d)", device, n);
  Context &c = ctx();
  if (c.device != device) {
    if (pipelines_busy() && c.device_set && hipSetDevice(c.device) == hipSuccess) {
      (void)pipeline_flush(c);   // volumes still pending or walked on the old device, in either instance: retire them there
      (void)pipelines_sync();
    }
    pipelines_forget(true);
    c.own_stream = nullptr;  // streams belong to a device; new ones are created lazily
    for (int l = 0; l < PRAD_MAX_LANES; l++) {
      if (c.lane_stream[l]) (void)hipStreamSynchronize(c.lane_stream[l]);
      c.lane_stream[l] = nullptr;
      c.lane_in[l] = nullptr;
    }
    c.event_pool.clear();
    c.events_used = 0;
  }
  c.device = device;
  c.device_set = true;
  PRAD_HIP(hipSetDevice(device));
  return PRAD_OK;
}
int prad_get_device(void) { return ctx().device; }

long long prad_workspace_bytes(void) {
  long long total = 0;
  for (const auto &kv : ctx().bufs) total += (long long)kv.second.cap;
  return total;
}
int prad_release_workspace(void) {
  Context &c = ctx();
  if (pipelines_busy()) {   // their buffers are about to go away: retire them first, in both instances
    (void)pipeline_flush(c);
    (void)pipelines_sync();
  }
  pipelines_forget(false);                // (what was known to be zero lived in the workspace)
  glszm_state_invalidate();               // its zone list lives in the workspace
  for (auto &kv : c.bufs) {
    if (kv.second.p) (void)hipFree(kv.second.p);
    kv.second.p = nullptr;
    kv.second.cap = 0;
  }
  (void)hipDeviceSynchronize();           // nothing may still read the buffers that go away
  for (auto &kv : c.pinned) {
    if (kv.second.p) (void)hipHostFree(kv.second.p);
    kv.second.p = nullptr;
    kv.second.cap = 0;
  }
  c.bufs.clear();
  c.pinned.clear();
  if (c.arena) (void)hipHostFree(c.arena);     // (the result arena: outstanding result views of this thread die with it)
  c.arena = nullptr;
  c.arena_pos = 0;
  release_image_queues();
  c.angles_cached.clear();   // (the cached angle tables and the deferred flag lived in the workspace)
  c.tables_cached.clear();
  StageRing &r = stage_ring();
  for (int i = 0; i < kStageRing; i++) {
    r.buf[i] = nullptr;
    r.busy[i] = false;
  }
  return PRAD_OK;
}

int prad_timing_begin(void) {
  Context &c = ctx();
  c.timing_only.clear();
  c.timing_accumulate = true;
  c.all_times.clear();
  c.all_calls.clear();
  c.events_used = 0;
  return PRAD_OK;
}
int prad_timing_begin_only(const char *kernel_family) {
  if (!kernel_family || !*kernel_family) return fail(PRAD_E_ARG, "timing: no kernel family named");
  int rc = prad_timing_begin();
  ctx().timing_only = kernel_family;
  return rc;
}
int prad_timing_count(const char *kernel_family) {
  Context &c = ctx();
  if (!kernel_family) return (int)c.all_calls.size();
  int n = 0;
  for (auto &t : c.all_times) n += t.family == kernel_family;
  return n;
}
int prad_timing_end(void) {
  Context &c = ctx();
  c.timing_only.clear();
  c.timing_accumulate = false;
  c.all_times.clear();
  c.all_calls.clear();
  return PRAD_OK;
}
int prad_timing_calls(void) { return (int)ctx().all_calls.size(); }
double prad_timing_ms(const char *family) {
  Context &c = ctx();
  double total = 0;
  if (!family) {
    for (auto &ab : c.all_calls) {
      float ms = 0;
      if (hipEventSynchronize(ab.second) != hipSuccess || hipEventElapsedTime(&ms, ab.first, ab.second) != hipSuccess) return -1.0;
      total += ms;
    }
    return total;
  }
  for (auto &t : c.all_times) {
    if (t.family != family) continue;
    float ms = 0;
    if (hipEventSynchronize(t.b) != hipSuccess || hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) return -1.0;
    total += ms;
  }
  return total;
}

int prad_set_deferred(int on) {
  Context &c = ctx();
  if (c.ensure_device() != PRAD_OK) return PRAD_E_HIP;
  if (on && !c.has("deferred_sticky")) {
    int *sticky = nullptr;   // first use on this device: a clean sticky flag (afterwards only the status query clears it)
    PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
    PRAD_HIP(hipMemset(sticky, 0, sizeof(int) * 16));
  }
  c.deferred = on != 0;
  return PRAD_OK;
}
int prad_set_lanes(int n) {
  Context &c = ctx();
  if (n < 0 || n > PRAD_MAX_LANES) return fail(PRAD_E_ARG, "lanes=%d outside [0, %d]", n, PRAD_MAX_LANES);
  if (pipelines_busy()) {   // (twin volumes share the lanes' streams: nothing of theirs stays behind)
    PRAD_TRY(c.ensure_device());
    PRAD_TRY(pipeline_flush(c));
    PRAD_TRY(pipelines_sync());
  }
  PRAD_TRY(c.lanes_sync());
  c.lanes = n;          // 0: back to the default (PRAD_LANES or 2) at the next deferred call
  c.lane_seq = 0;
  return PRAD_OK;
}
int prad_set_deferred_mode(int mode) {
  if (mode < -1 || mode > 1) return fail(PRAD_E_ARG, "deferred mode %d (0 lanes, 1 pipeline, -1 environment default)", mode);
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  PRAD_TRY(pipeline_flush(c));
  PRAD_TRY(pipelines_sync());
  PRAD_TRY(c.lanes_sync());
  pipelines().mode = mode;
  return PRAD_OK;
}
int prad_set_workspace(int id) {
  if (id < 0 || id > 7) return fail(PRAD_E_ARG, "workspace %d outside [0, 7]", id);
  ctx().workspace = id;
  return PRAD_OK;
}
int prad_result_alloc(size_t bytes, void **out) {
  if (!out) return fail(PRAD_E_ARG, "result_alloc: out is NULL");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  return c.arena_alloc(bytes, out);
}
int prad_deferred_join(void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  PRAD_TRY(pipeline_flush(c));
  PRAD_TRY(pipelines_order((hipStream_t)stream));   // the flushed work of either instance sits on the stream of its pack
  return c.lanes_join((hipStream_t)stream);
}
int prad_deferred_mark(int *flag, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!flag || !c.in_arena(flag, sizeof(int))) return fail(PRAD_E_ARG, "deferred_mark: flag must lie in the result arena");
  PRAD_TRY(pipeline_flush(c));
  PRAD_TRY(pipelines_order((hipStream_t)stream));   // the copy of the verdict word stands behind both instances
  int *sticky = nullptr;
  PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
  PRAD_HIP(hipMemcpyAsync(flag, sticky, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return PRAD_OK;
}
int prad_deferred_status(void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  PRAD_TRY(pipeline_flush(c));
  PRAD_TRY(pipelines_sync());
  PRAD_HIP(hipStreamSynchronize((hipStream_t)stream));
  PRAD_TRY(c.lanes_sync());
  if (!c.has("deferred_sticky")) return PRAD_OK;  // no deferred call yet
  int *sticky = nullptr;
  PRAD_TRY(c.get<int>("deferred_sticky", 16, &sticky));
  // (on the caller's stream, through pinned memory: a plain hipMemcpy is a null-stream operation that waits for the
  // whole device -- with six case threads each asking once per derived image it serialised the batch, 65 -> 37 cases/s)
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned("sticky_h", 64, &pin));
  PRAD_HIP(hipMemcpyAsync(pin, sticky, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  PRAD_HIP(hipStreamSynchronize((hipStream_t)stream));
  const int h = *(const int *)pin;
  if (h) {
    PRAD_HIP(hipMemsetAsync(sticky, 0, sizeof(int), (hipStream_t)stream));
    PRAD_HIP(hipStreamSynchronize((hipStream_t)stream));
    return fail(PRAD_E_DEFERRED, "a deferred GLCM/GLRLM call saw masked levels outside [1, Ng]; repeat it synchronously");
  }
  return PRAD_OK;
}

double prad_last_device_ms(void) {
  Context &c = ctx();
  if (!c.call_timed) return -1.0;
  float ms = 0;
  if (hipEventElapsedTime(&ms, c.call_a, c.call_b) != hipSuccess) return -1.0;
  return ms;
}

double prad_last_kernel_ms(const char *family) {
  Context &c = ctx();
  double total = 0;
  bool any = false;
  for (auto &t : c.times) {
    if (family && t.family != family) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, t.a, t.b) != hipSuccess) return -1.0;
    total += ms;
    any = true;
  }
  return any ? total : -1.0;
}

int prad_get_angle_count(const int *size, const int *distances, int Nd, int Ndist, int bidirectional,
                         int force2Ddim) {
  if (!size || !distances || Nd < 1 || Ndist < 1) return 0;
  return angle_count(size, distances, Nd, Ndist, bidirectional, force2Ddim);
}

int prad_build_angles(const int *size, const int *distances, int Nd, int Ndist, int force2Ddim, int Na,
                      int *angles) {
  if (!size || !distances || !angles || Nd < 1 || Ndist < 1) return 1;
  return angle_build(size, distances, Nd, Ndist, force2Ddim, Na, angles);
}

// The sweep plan of a segment-mode GLCM / GLRLM call as ints (the record's order: include/pyradiomics_amd.h).  Host only.
int prad_debug_sweep_plan(const int *size, int Nd, const int *angles, int Na, int Ng, int Nr, int want_glcm, int want_glrlm,
                          int cus, int *out, int cap) {
  if (!size || !angles || !out || Nd < 1 || Nd > PRAD_MAX_ND || Na < 1 || cap < 1) return 0;
  for (int d = 0; d < Nd; d++)
    if (size[d] < 1) return 0;
  PlanInput in;
  in.nd = Nd;
  in.size = size;
  in.angles = angles;
  in.Na = Na;
  in.Ng = Ng;
  in.Nr = Nr;
  in.want_glcm = want_glcm != 0;
  in.want_glrlm = want_glrlm != 0;
  const SweepPlan p = plan_sweep(in, sweep_knobs_from_env(), cus > 0 ? cus : cu_count());
  std::vector<int> r;
  r.push_back(p.ok ? 1 : 0);
  if (p.ok) {
    for (int v : {p.Nz, p.Ny, p.Nx, (int)p.fused, (int)p.fw, (int)p.fw2, (int)p.fw2_rows, p.RS, p.RSr, p.RSfw, p.RSfw_rows, p.RS2,
                  p.RS2r, (int)p.LONG, (int)p.LONGr, (int)p.LONGfw, (int)p.LONGfw2, (int)p.LONGfw2r, (int)p.lds_bytes,
                  (int)p.lds_bytes_rows, (int)p.lds_fw, (int)p.lds_fw_rows, (int)p.lds_fw2, (int)p.lds_fw2_rows, p.threads,
                  p.fw_threads, p.fw_rows_threads, p.fwK, p.fw_blocks, p.fw2_copies, p.fw2r_copies, p.fw2r_waves, p.LPL, p.pitch,
                  p.padw, p.pitch16, (int)p.vec_rows, (int)p.skip1, p.row_slot, p.fw_xblocks, p.lines.count})
      r.push_back(v);
    for (int i = 0; i < p.lines.count; i++) {
      const SweepDesc &D = p.lines.d[i];
      for (int v : {D.slot, D.NM, D.NU, D.NX, D.du, D.dx, (int)D.sM, (int)D.sU, D.LXc, (int)D.chunks}) r.push_back(v);
    }
    r.push_back(p.aset.count);
    for (int a = 0; a < p.aset.count; a++)
      for (int d = 0; d < 3; d++) r.push_back(p.aset.off[a][d]);
    r.push_back((p.fw || p.fw2) ? 1 : 0);
    if (p.fw || p.fw2) {   // (the planner fills the set only for a fixed-window launch)
      const FwSet &f = p.fwset;
      for (int v : {f.count, f.NX, f.pitch, f.nrows, f.xcd}) r.push_back(v);
      for (int i = 0; i < PRAD_MAX_SWEEP + 1; i++) r.push_back(f.first_block[i]);
      for (int v : {f.xslot, f.xRS, f.xwaves, f.xgpd}) r.push_back(v);
      for (int i = 0; i < f.count; i++) {
        const FwDesc &D = f.d[i];
        for (int v : {D.slot, D.NM, D.NU, D.du, D.dx, (int)D.sM, (int)D.sU, D.CL, D.pieces, D.chunks, D.dom_kind}) r.push_back(v);
      }
    }
  }
  if ((int)r.size() > cap) return -(int)r.size();
  std::copy(r.begin(), r.end(), out);
  return (int)r.size();
}

// The launches the deferred pipeline plans for a script of events, replayed through a fresh planner (the layouts of an event and
// of a record: include/pyradiomics_amd.h).  Host only.
int prad_debug_pipe_plan(const long long *events, int nevents, int *out, int cap) {
  if (!events || nevents < 1 || !out || cap < 1) return 0;
  std::vector<int> r;
  pipe_replay(events, nevents, r);
  if ((int)r.size() > cap) return -(int)r.size();
  std::copy(r.begin(), r.end(), out);
  return (int)r.size();
}

// The pairs tier of a segment-mode GLDM / NGTDM call as ints (the record's order: include/pyradiomics_amd.h).  Host only.
int prad_debug_neigh_plan(const int *size, int Nd, const int *angles, int Na, int Ng, int ngtdm, int knobs, int cus, int *out, int cap) {
  if (!size || !angles || !out || Nd < 1 || Nd > PRAD_MAX_ND || Na < 1 || Ng < 1 || cap < 1) return 0;
  for (int d = 0; d < Nd; d++)
    if (size[d] < 1) return 0;
  const PairsNeighInput in = {Nd, size, angles, Na, Ng, ngtdm != 0, false};
  const NeighKnobs kn = {(knobs & 1) != 0, (knobs & 2) != 0};
  const PairsNeighPlan p = plan_pairs_neigh(in, kn, cus > 0 ? cus : cu_count());
  const int r[] = {(int)p.applies, p.variant, (int)p.box, (int)p.narrow, p.mode, (int)p.lds, (int)p.threads, (int)p.grid,
                   (int)p.box_grid, p.dims[0], p.dims[1], p.dims[2], p.rad[0], p.rad[1], p.rad[2]};
  const int n = (int)(sizeof(r) / sizeof(r[0]));
  if (n > cap) return -n;
  std::copy(r, r + n, out);
  return n;
}

// ---- GLCM / GLRLM ---------------------------------------------------------------------------
int prad_calculate_glcm_glrlm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                  const int *angles, int Na, int Ng, int Nr, int Nvox, const int *voxels,
                                  int kernelRadius, int force2Ddim, double *glcm, double *glrlm, void *stream) {
  return texture_pairs_runs(image, mask, size, Nd, angles, Na, Ng, Nr, Nvox, voxels, kernelRadius, force2Ddim, glcm,
                            glrlm, (hipStream_t)stream);
}
int prad_calculate_glcm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                            int Na, int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                            double *glcm, void *stream) {
  if (!glcm) return fail(PRAD_E_ARG, "glcm is NULL");
  return texture_pairs_runs(image, mask, size, Nd, angles, Na, Ng, 1, Nvox, voxels, kernelRadius, force2Ddim, glcm,
                            nullptr, (hipStream_t)stream);
}
int prad_calculate_glrlm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                             int Na, int Ng, int Nr, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             double *glrlm, void *stream) {
  if (!glrlm) return fail(PRAD_E_ARG, "glrlm is NULL");
  return texture_pairs_runs(image, mask, size, Nd, angles, Na, Ng, Nr, Nvox, voxels, kernelRadius, force2Ddim,
                            nullptr, glrlm, (hipStream_t)stream);
}

int prad_calculate_glcm_glrlm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                              int Na, int Ng, int Nr, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                              double *glcm, double *glrlm) {
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  if (Ng < 1 || Nvox < 1 || Na < 1) return fail(PRAD_E_ARG, "Ng/Nvox/Na must be >= 1");
  const size_t nglcm = glcm ? (size_t)Nvox * Ng * Ng * Na : 0;
  const size_t nglrlm = glrlm ? (size_t)Nvox * Ng * (size_t)std::max(Nr, 1) * Na : 0;
  double *d_glcm = nullptr, *d_glrlm = nullptr;
  if (glcm) PRAD_TRY(fetch_output(c, "o_glcm", glcm, nglcm, &d_glcm));
  if (glrlm) PRAD_TRY(fetch_output(c, "o_glrlm", glrlm, nglrlm, &d_glrlm));
  int rc = texture_pairs_runs(st.image, st.mask, size, Nd, angles, Na, Ng, Nr, Nvox, st.voxels, kernelRadius,
                              force2Ddim, d_glcm, d_glrlm, c.own_stream);
  if (rc != PRAD_OK) return rc;
  if (glcm) PRAD_TRY(copy_back(c, glcm, d_glcm, nglcm));
  if (glrlm) PRAD_TRY(copy_back(c, glrlm, d_glrlm, nglrlm));
  return PRAD_OK;
}
int prad_calculate_glcm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                        int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, double *glcm) {
  if (!glcm) return fail(PRAD_E_ARG, "glcm is NULL");
  return prad_calculate_glcm_glrlm(image, mask, size, Nd, angles, Na, Ng, 1, Nvox, voxels, kernelRadius, force2Ddim,
                                   glcm, nullptr);
}
int prad_calculate_glrlm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                         int Na, int Ng, int Nr, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         double *glrlm) {
  if (!glrlm) return fail(PRAD_E_ARG, "glrlm is NULL");
  return prad_calculate_glcm_glrlm(image, mask, size, Nd, angles, Na, Ng, Nr, Nvox, voxels, kernelRadius, force2Ddim,
                                   nullptr, glrlm);
}

// ---- GLDM -----------------------------------------------------------------------------------
int prad_calculate_gldm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                            int Na, int Ng, int alpha, int Nvox, const int *voxels, int kernelRadius,
                            int force2Ddim, double *gldm, void *stream) {
  return texture_gldm(image, mask, size, Nd, angles, Na, Ng, alpha, Nvox, voxels, kernelRadius, force2Ddim, gldm,
                      (hipStream_t)stream);
}
int prad_calculate_gldm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                        int Ng, int alpha, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                        double *gldm) {
  if (!gldm) return fail(PRAD_E_ARG, "gldm is NULL");
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  if (Ng < 1 || Nvox < 1 || Na < 1) return fail(PRAD_E_ARG, "Ng/Nvox/Na must be >= 1");
  const size_t n = (size_t)Nvox * Ng * (2 * (size_t)Na + 1);
  double *d = nullptr;
  PRAD_TRY(fetch_output(c, "o_gldm", gldm, n, &d));
  int rc = texture_gldm(st.image, st.mask, size, Nd, angles, Na, Ng, alpha, Nvox, st.voxels, kernelRadius,
                        force2Ddim, d, c.own_stream);
  if (rc != PRAD_OK) return rc;
  return copy_back(c, gldm, d, n);
}

int prad_calculate_gldm_ngtdm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                                  int Na, int Ng, int alpha, double *gldm, double *ngtdm, void *stream) {
  return texture_gldm_ngtdm(image, mask, size, Nd, angles, Na, Ng, alpha, gldm, ngtdm, (hipStream_t)stream);
}

// ---- NGTDM ----------------------------------------------------------------------------------
int prad_calculate_ngtdm_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                             int Na, int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             double *ngtdm, void *stream) {
  return texture_ngtdm(image, mask, size, Nd, angles, Na, Ng, Nvox, voxels, kernelRadius, force2Ddim, ngtdm,
                       (hipStream_t)stream);
}
int prad_calculate_ngtdm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                         int Na, int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         double *ngtdm) {
  if (!ngtdm) return fail(PRAD_E_ARG, "ngtdm is NULL");
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  if (Ng < 1 || Nvox < 1 || Na < 1) return fail(PRAD_E_ARG, "Ng/Nvox/Na must be >= 1");
  const size_t n = (size_t)Nvox * Ng * 3;
  double *d = nullptr;
  PRAD_TRY(fetch_output(c, "o_ngtdm", ngtdm, n, &d));
  int rc = texture_ngtdm(st.image, st.mask, size, Nd, angles, Na, Ng, Nvox, st.voxels, kernelRadius, force2Ddim, d,
                         c.own_stream);
  if (rc != PRAD_OK) return rc;
  return copy_back(c, ngtdm, d, n);
}

// ---- plane-range accumulators (one segment over several GPUs) ------------------------------
int prad_neigh_accumulate_dev(int family, const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                              const int *angles, int Na, int Ng, int alpha, int z_lo, int z_hi, long long *acc,
                              void *stream) {
  return neigh_accumulate_i64(family, image, mask, size, Nd, angles, Na, Ng, alpha, z_lo, z_hi, acc,
                              (hipStream_t)stream);
}
int prad_neigh_finalize_dev(int family, const long long *acc, int Ng, int Na, double *out, void *stream) {
  return neigh_finalize_i64(family, acc, Ng, Na, out, (hipStream_t)stream);
}

// ---- GLSZM: the host-array wrappers (staging lives here; the entry points for device arrays: prad_glszm.hip) ----
int prad_calculate_glszm(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                         int Na, int Ng, int Ns, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                         long long *nzones) {
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  return prad_calculate_glszm_dev(st.image, st.mask, size, Nd, angles, Na, Ng, Ns, Nvox, st.voxels, kernelRadius,
                                  force2Ddim, nzones, c.own_stream);
}
int prad_fill_glszm(double *glszm, int Nvox, int Ng, int maxRegion) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!glszm || Ng < 1 || maxRegion < 1 || Nvox < 1) return fail(PRAD_E_ARG, "bad fill_glszm arguments");
  const size_t n = (size_t)Nvox * Ng * maxRegion;
  double *d = nullptr;
  PRAD_TRY(c.get<double>("o_glszm", n, &d));
  PRAD_TRY(prad_fill_glszm_dev(d, Nvox, Ng, maxRegion, c.own_stream));
  return copy_back(c, glszm, d, n);
}
// ---- fused voxel-based GLCM features -----------------------------------------------------------
int prad_voxel_glcm_features_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                 const int *angles, int Na, int Ng, int Nvox, const int *voxels, int kernelRadius,
                                 int force2Ddim, int symmetric, const int *feature_ids, int nfeat, double *out,
                                 uint32_t *empty_mask, uint32_t *any_nonempty, void *stream) {
  return voxel_glcm_features_dev(image, mask, size, Nd, angles, Na, Ng, Nvox, voxels, kernelRadius, force2Ddim,
                                 symmetric, feature_ids, nfeat, out, empty_mask, any_nonempty, (hipStream_t)stream);
}
int prad_voxel_glcm_features(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles,
                             int Na, int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim,
                             int symmetric, const int *feature_ids, int nfeat, double *out, uint32_t *empty_mask,
                             uint32_t *any_nonempty) {
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  if (!voxels || !out || nfeat < 1) return fail(PRAD_E_ARG, "voxel_glcm: bad arguments");
  double *d_out = nullptr;
  unsigned *d_masks = nullptr;
  PRAD_TRY(c.get<double>("o_vox", (size_t)nfeat * Nvox, &d_out));
  PRAD_TRY(c.get<unsigned>("o_voxmask", (size_t)Nvox + 1, &d_masks));
  int rc = voxel_glcm_features_dev(st.image, st.mask, size, Nd, angles, Na, Ng, Nvox, st.voxels, kernelRadius,
                                   force2Ddim, symmetric, feature_ids, nfeat, d_out, d_masks + 1, d_masks, c.own_stream);
  if (rc != PRAD_OK) return rc;
  PRAD_TRY(copy_back(c, out, d_out, (size_t)nfeat * Nvox));
  if (empty_mask) PRAD_HIP(hipMemcpy(empty_mask, d_masks + 1, sizeof(unsigned) * Nvox, hipMemcpyDeviceToHost));
  if (any_nonempty) PRAD_HIP(hipMemcpy(any_nonempty, d_masks, sizeof(unsigned), hipMemcpyDeviceToHost));
  return PRAD_OK;
}

__global__ void flag_to_double_kernel(const int *__restrict__ flag, double *__restrict__ out) { out[0] = flag[0] ? 1.0 : 0.0; }

int prad_glcm_mcc_dev(const double *glcm, int Ng, int Na, int symmetric, double *out, void *stream) {
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  if (!glcm || !out || Ng < 1 || Na < 1) return fail(PRAD_E_ARG, "glcm_mcc: bad arguments");
  const int nmax = std::min(Ng, PRAD_MCC_NMAX);
  size_t lds = mcc_scratch_bytes(Ng, nmax);
  if (lds > 150 * 1024) return fail(PRAD_E_UNSUPPORTED, "glcm_mcc: Ng=%d exceeds the LDS scratch", Ng);
  const size_t staged_lds = ((lds + 15) & ~(size_t)15) + sizeof(double) * (size_t)Ng * Ng;   // + the angle's counts
  const int staged = staged_lds <= 150 * 1024;
  if (staged) lds = staged_lds;
  hipStream_t s = (hipStream_t)stream;
  double *d_out = nullptr;
  int *d_flag = nullptr;
  PRAD_TRY(c.get<double>("mcc_out", (size_t)Na + 1, &d_out));
  PRAD_TRY(c.get<int>("mcc_flag", 4, &d_flag));
  PRAD_HIP(hipMemsetAsync(d_flag, 0, sizeof(int) * 4, s));
  {
    Timed t(c, "features", s);
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&glcm_matrix_mcc_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(glcm_matrix_mcc_kernel, dim3(Na), dim3(PRAD_MCC_BT), lds, s, glcm, Ng, Na, symmetric, nmax, staged, d_out, d_flag);
    PRAD_TRY(check_launch("glcm_matrix_mcc_kernel"));
  }
  if (c.deferred && c.in_arena(out, sizeof(double) * ((size_t)Na + 1))) {
    // enqueue only: out[Na] tells afterwards whether more than PRAD_MCC_NMAX levels occurred (then out[0..Na) is void)
    hipLaunchKernelGGL(flag_to_double_kernel, dim3(1), dim3(1), 0, s, (const int *)d_flag, d_out + Na);
    PRAD_TRY(check_launch("flag_to_double_kernel"));
    PRAD_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * ((size_t)Na + 1), hipMemcpyDeviceToHost, s));
    return PRAD_OK;
  }
  void *pin = nullptr;
  PRAD_TRY(c.get_pinned("mcc_pin", sizeof(double) * ((size_t)Na + 2), &pin));
  hipLaunchKernelGGL(flag_to_double_kernel, dim3(1), dim3(1), 0, s, (const int *)d_flag, d_out + Na);
  PRAD_TRY(check_launch("flag_to_double_kernel"));
  PRAD_HIP(hipMemcpyAsync(pin, d_out, sizeof(double) * ((size_t)Na + 1), hipMemcpyDeviceToHost, s));
  PRAD_HIP(hipStreamSynchronize(s));
  memcpy(out, pin, sizeof(double) * Na);
  const int flag = ((const double *)pin)[Na] != 0.0;
  if (flag) return fail(PRAD_E_UNSUPPORTED, "glcm_mcc: more than %d grey levels occur; use the host route", PRAD_MCC_NMAX);
  return PRAD_OK;
}

int prad_voxel_glcm_mcc_dev(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                            int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, int symmetric,
                            double *out, void *stream) {
  return voxel_glcm_mcc_dev(image, mask, size, Nd, angles, Na, Ng, Nvox, voxels, kernelRadius, force2Ddim, symmetric, out,
                            (hipStream_t)stream);
}
int prad_voxel_glcm_mcc(const int32_t *image, const uint8_t *mask, const int *size, int Nd, const int *angles, int Na,
                        int Ng, int Nvox, const int *voxels, int kernelRadius, int force2Ddim, int symmetric, double *out) {
  Context &c = ctx();
  Staged st;
  PRAD_TRY(stage_inputs(c, image, mask, size, Nd, Nvox, voxels, &st));
  if (!voxels || !out) return fail(PRAD_E_ARG, "voxel_glcm_mcc: bad arguments");
  double *d_out = nullptr;
  PRAD_TRY(c.get<double>("o_mcc", (size_t)Nvox, &d_out));
  int rc = voxel_glcm_mcc_dev(st.image, st.mask, size, Nd, angles, Na, Ng, Nvox, st.voxels, kernelRadius, force2Ddim,
                              symmetric, d_out, c.own_stream);
  if (rc != PRAD_OK) return rc;
  return copy_back(c, out, d_out, (size_t)Nvox);
}

int prad_voxel_texture_features_dev(int family, const int32_t *image, const uint8_t *mask, const int *size, int Nd,
                                    const int *angles, int Na, int Ng, int alpha, int Nvox, const int *voxels,
                                    int kernelRadius, int force2Ddim, const int *feature_ids, int nfeat, double *out,
                                    void *stream) {
  return voxel_texture_features_dev(family, image, mask, size, Nd, angles, Na, Ng, alpha, Nvox, voxels, kernelRadius,
                                    force2Ddim, feature_ids, nfeat, out, (hipStream_t)stream);
}

}  // extern "C"
