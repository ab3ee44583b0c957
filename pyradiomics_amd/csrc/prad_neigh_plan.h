// prad_neigh_plan.h -- the pairs tier of a GLDM / NGTDM call (kernels_pairs.h: the 16-bit level volume, between the byte kernels
// of kernels_neigh.h and the exact kernels): whether it applies and with what launch, as a pure function of the call's shape, its
// HOST angle list, the switches and the CU count.  No Context, no HIP header, no environment.  pairs_neigh in prad_api.hip
// executes the plan and decides nothing of its own; prad_debug_neigh_plan records it and tests/test_neigh_route_plan.py holds it
// to tests/neigh_reference.expected_route and to the u32 overflow rule without a device.  The byte tier, the order of the tiers
// and the deferred rule stay with texture_gldm / texture_ngtdm and kernels_neigh.h.
//
// The volume is embedded in 3-D (leading extents 1); nacc = Ng * (Na + 1) bins.
//   applies  segment mode, Nd <= 3, 1 <= Ng <= 65535, fewer than 2^31 - 1 voxels, the table's offsets within +-127, bins within
//            1 GiB as u64, Na <= 128 unless box, not with no_pairs
//   box      NGTDM whose offsets are a whole box around the voxel (cube - 1 == Na distinct non-zero offsets inside it) with cube <=
//            4096, not with no_box: separable box sums; narrow (32-bit words) with cube <= 127
//   mode     where the bins live: 1 LDS (GLDM u32, NGTDM u64) within 150 KB; 2 NGTDM as u32 in LDS under a grid fine enough that
//            a workgroup's sums stay below 2^32; 0 global memory
#pragma once
#include <algorithm>
#include <cstdlib>

namespace prad {

constexpr int kPairMaxAngles = 128;              // PRAD_PAIR_MAXA (static_assert in prad_api.hip)
constexpr size_t kPairLdsBytes = 150 * 1024;     // PRAD_PAIR_LDS_WORDS u32

struct NeighKnobs { bool no_pairs = false, no_box = false; };   // PRAD_NO_PAIRS, PRAD_NGTDM_NO_BOX

struct PairsNeighInput {
  int nd;
  const int *size, *angles;       // host: [nd], [Na][nd]
  int Na, Ng;
  bool ngtdm, voxel_mode;
};

// prad_last_variant() of the tier: 0 "none" (it does not apply), else 1 + 3 * placement + box word
constexpr int kPairsVariants = 10;
inline const char *pairs_variant_name(int v) {
  static const char *const names[kPairsVariants] = {"none", "pairs-global", "pairs-global+box32", "pairs-global+box64", "pairs-lds64",
                                                    "pairs-lds64+box32", "pairs-lds64+box64", "pairs-lds32", "pairs-lds32+box32",
                                                    "pairs-lds32+box64"};
  return names[v >= 0 && v < kPairsVariants ? v : 0];
}

struct PairsNeighPlan {
  bool applies = false, box = false, narrow = false;
  int dims[3] = {1, 1, 1};   // Nz Ny Nx
  long long n = 1;
  int na = 0;                               // min(Na, 128) offsets of the table, embedded (the box path needs the radii only)
  signed char o[kPairMaxAngles][4] = {};
  int rad[3] = {0, 0, 0};                   // the largest |offset| per axis
  int mode = 0, variant = 0;
  size_t lds = 0;                           // dynamic LDS of the bin kernel
  unsigned threads = 0, grid = 0;           // of the bin kernel (pairs_neigh_kernel / pairs_ngtdm_box_kernel)
  unsigned box_grid = 0;                    // of the two box-axis launches
};

inline PairsNeighPlan plan_pairs_neigh(const PairsNeighInput &in, const NeighKnobs &kn, int cus) {
  PairsNeighPlan p;
  const int nd = in.nd, Na = in.Na, Ng = in.Ng;
  if (in.voxel_mode || nd > 3 || Ng < 1 || Ng > 65535 || Na < 1 || kn.no_pairs) return p;
  for (int d = 0; d < nd; d++) p.n *= (p.dims[3 - nd + d] = in.size[d]);
  if (p.n >= 0x7fffffffLL) return p;
  p.na = std::min(Na, kPairMaxAngles);
  bool fit = true;    // the table's offsets fit a signed char
  for (int a = 0; a < Na; a++)
    for (int d = 0; d < nd; d++) {
      const int o = in.angles[a * nd + d], e = 3 - nd + d;
      p.rad[e] = std::max(p.rad[e], std::abs(o));
      if (a >= p.na) continue;
      fit = fit && o >= -127 && o <= 127;
      p.o[a][e] = (signed char)o;
    }
  // NGTDM over a FULL box of neighbours (distances [1], [1, 2], [1, 2, 3] ...; in-plane boxes under force2D): decided on the
  // host's angle list.  (Each 2 r + 1 of a cube <= 4096 is below 4096; the earlier forms of this test also asked for
  // cube * Ng < 2^40, and for narrow words cube * Ng < 2^24: with Ng <= 65535 neither can fail -- the products stay below 2^28
  // and 2^23 -- so they are not asked here.)
  long long cube = 1;
  bool box = in.ngtdm && !kn.no_box && std::max(p.rad[0], std::max(p.rad[1], p.rad[2])) < 2048;
  if (box) {
    cube = (long long)(2 * p.rad[0] + 1) * (2 * p.rad[1] + 1) * (2 * p.rad[2] + 1);
    box = cube - 1 == Na && cube <= 4096;
  }
  if (box) {        // cube - 1 distinct non-zero offsets inside the cube are the whole cube
    bool seen[4096] = {};
    for (int a = 0; box && a < Na; a++) {
      long long idx = 0;
      for (int d = 0; d < 3; d++) idx = idx * (2 * p.rad[d] + 1) + ((d < 3 - nd ? 0 : in.angles[a * nd + d - (3 - nd)]) + p.rad[d]);
      if (idx == cube / 2 || seen[idx]) box = false;      // (the centre of the cube is the zero offset)
      seen[idx] = true;
    }
  }
  const size_t nacc = (size_t)Ng * ((size_t)Na + 1);
  if ((!box && Na > kPairMaxAngles) || !fit || nacc * 8 > ((size_t)1 << 30)) return p;
  p.applies = true;
  p.box = box;
  p.narrow = box && cube <= 127;      // (ROI voxels << 24 | level sum) fits 32 bits
  // bins in LDS when they fit 150 KB: GLDM u32; NGTDM u64, or u32 with a grid fine enough that a workgroup's sums
  // (voxels x angles x Ng at most) stay below 2^32
  p.mode = nacc * (in.ngtdm ? 8 : 4) <= kPairLdsBytes ? 1 : (in.ngtdm && nacc * 4 <= kPairLdsBytes) ? 2 : 0;
  p.lds = p.mode == 0 ? 0 : nacc * (p.mode == 1 && in.ngtdm ? 8 : 4);
  // bins beyond 40 KB: one workgroup per CU, so make it a 16-wave one (4 waves per CU left the neighbour gathers
  // latency-bound: GLDM at 300 levels x 124 angles took 7.8 ms)
  const long long bt = (p.mode && p.lds > 40 * 1024) ? 1024 : 256;
  long long want = (long long)cus * (bt == 1024 ? 1 : 16);
  if (p.mode == 2) {      // voxels per workgroup <= 2^32 / (Na * Ng) / 2
    const long long cap = std::max<long long>(1, (1LL << 31) / ((long long)Na * Ng));
    want = std::max(want, (p.n + cap - 1) / cap);
  }
  p.threads = (unsigned)bt;
  p.grid = (unsigned)std::max<long long>(1, std::min<long long>((p.n + bt - 1) / bt, want));
  p.box_grid = (unsigned)std::max<long long>(1, std::min<long long>((p.n + 255) / 256, (long long)cus * 32));
  // (the label names the LDS bin width: GLDM's are u32)
  p.variant = 1 + 3 * (!in.ngtdm && p.mode ? 2 : p.mode) + (box ? (p.narrow ? 1 : 2) : 0);
  return p;
}

}  // namespace prad
