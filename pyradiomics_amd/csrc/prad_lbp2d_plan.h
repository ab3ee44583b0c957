// prad_lbp2d_plan.h -- how an LBP2D call (kernels_lbp2d.h, kernels_batch_lbp2d.h) is cut into workgroups: the tile of output
// voxels, the block of cells staged around it, the grid, the LDS bytes and a verdict, as a pure function of the extents, the axis
// the planes are stacked along (force2Ddimension) and the halo ceil(R).  No Context, no HIP header, no environment.
// prad_lbp2d_dev / prad_batch_lbp2d_dev execute the plan and decide nothing of their own; prad_lbp2d_plan and
// prad_batch_lbp2d_plan hand it out and tests/test_lbp2d_plan.py holds it to "every output voxel exactly once" without a device.
//
// The volume is [nz][ny][nx].  A plane is arr.swapaxes(0, axis)[idx]:
//   axis 0   plane z, rows y, cols x        axis 1   plane y, rows z, cols x        axis 2   plane x, rows y, cols z
// A tile is a block [tz][ty][tx] of OUTPUT voxels, every extent a power of two; the staged block adds `halo` cells on both sides
// of the two in-plane axes and nothing along the plane axis (planes do not see one another).  x is the fastest axis of the tile
// and of the staged block for EVERY axis: lanes run over x, so global loads and stores are coalesced along x and the four
// corners of a sample are lane-consecutive LDS reads -- for axis 2, where x is the plane axis, that means each lane owns a plane
// of its own.
//   axes 0, 1   tx = min(64, p2(nx)); rows = min(p2(rows of the volume), 1024 / tx, 32); planes = min(p2(planes), 1024 / (tx rows), 8)
//   axis 2      tz = min(8, p2(nz)), ty = min(8, p2(ny)), tx = min(64, p2(nx))
// then, while the staged block (float64 cells) is above the LDS budget, one extent is halved: the planes first (axis 2: the
// cols down to 4), then the rows down to 4, then tx down to 8, then whatever is left.  The budget is 40 KiB: four workgroups of
// 256 threads share the 160 KiB of a CU.
#pragma once
#include <algorithm>

namespace prad {

constexpr int kLbpMaxHalo = 8;                    // ceil(R) of the native domain
constexpr int kLbpMaxSamples = 24;                // P of the native domain (the codes of `default` fit a float32 exactly)
constexpr int kLbpThreads = 256;
constexpr long long kLbpLdsBudget = 40 * 1024;
constexpr long long kLbpMaxGroups = 2147483647LL; // workgroups of one launch (grid x)

// verdicts
constexpr int kLbpNative = 0;
constexpr int kLbpHalo = 1;                       // halo outside [0, kLbpMaxHalo]: the host route
constexpr int kLbpGrid = 2;                       // more workgroups than one launch holds: the host route

struct Lbp2dPlan {
  int verdict = kLbpNative;
  int tile[3] = {1, 1, 1};          // tz ty tx: output voxels of a workgroup
  int staged[3] = {1, 1, 1};        // the cells it stages
  long long tiles[3] = {0, 0, 0};   // tiles along z, y, x
  long long groups = 0;             // workgroups of the launch (the batch: the items)
  long long lds = 0;                // bytes of dynamic LDS
};

inline int lbp_p2(int n) {          // the smallest power of two >= n (n >= 1)
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

inline bool lbp_in_plane(int axis, int d) { return d != axis; }

// tile and staged block for extents ext[3] (>= 1 each); -> false when nothing fits the budget (never within the halo domain)
inline bool lbp2d_tile(const int *ext, int axis, int halo, Lbp2dPlan *p) {
  int *t = p->tile;
  t[2] = std::min(64, lbp_p2(ext[2]));
  // shrink order: indices into t[], each with the extent it is halved down to in the first round
  int order[3], floor1[3];
  if (axis == 2) {
    t[0] = std::min(8, lbp_p2(ext[0]));
    t[1] = std::min(8, lbp_p2(ext[1]));
    order[0] = 0, floor1[0] = 4;      // cols (z)
    order[1] = 2, floor1[1] = 8;      // planes (x): the lanes
    order[2] = 1, floor1[2] = 4;      // rows (y)
  } else {
    const int rows = axis == 0 ? 1 : 0, planes = axis == 0 ? 0 : 1;
    const int rem = 1024 / t[2];
    t[rows] = std::min(lbp_p2(ext[rows]), std::min(rem, 32));
    t[planes] = std::min(lbp_p2(ext[planes]), std::min(rem / t[rows], 8));
    order[0] = planes, floor1[0] = 1;
    order[1] = rows, floor1[1] = 4;
    order[2] = 2, floor1[2] = 8;
  }
  auto bytes = [&]() {
    long long n = 8;
    for (int d = 0; d < 3; d++) n *= (p->staged[d] = t[d] + (lbp_in_plane(axis, d) ? 2 * halo : 0));
    return n;
  };
  for (int round = 0; round < 2; round++)
    for (int k = 0; k < 3; k++)
      while (bytes() > kLbpLdsBudget && t[order[k]] > (round ? 1 : floor1[k])) t[order[k]] >>= 1;
  p->lds = bytes();
  return p->lds <= kLbpLdsBudget;
}

// one volume
inline Lbp2dPlan lbp2d_plan(const int *size, int axis, int halo) {
  Lbp2dPlan p;
  if (halo < 0 || halo > kLbpMaxHalo || !lbp2d_tile(size, axis, halo, &p)) {
    p.verdict = kLbpHalo;
    return p;
  }
  p.groups = 1;
  for (int d = 0; d < 3; d++) p.groups *= (p.tiles[d] = ((long long)size[d] + p.tile[d] - 1) / p.tile[d]);
  if (p.groups > kLbpMaxGroups) p.verdict = kLbpGrid;
  return p;
}

// one workgroup of the batched launch: the tile of ROI `roi` whose first output voxel is (z0, y0, x0) of the box.  Also the row
// of the table prad_batch_lbp2d_plan hands out (4 int32).
struct BatchLbpItem {
  int roi, z0, y0, x0;
};
static_assert(sizeof(BatchLbpItem) == 16, "BatchLbpItem is 4 int32");

// a batch of boxes (sizes [B][3], checked >= 1): ONE tile shape for the launch, that of the largest extent per axis; the items
// list the tiles of every box, boxes in their order, x fastest.  items may be NULL (count only).
inline Lbp2dPlan batch_lbp2d_plan(const int *sizes, int B, int axis, int halo, BatchLbpItem *items) {
  Lbp2dPlan p;
  int ext[3] = {1, 1, 1};
  for (int b = 0; b < B; b++)
    for (int d = 0; d < 3; d++) ext[d] = std::max(ext[d], sizes[3 * b + d]);
  if (halo < 0 || halo > kLbpMaxHalo || !lbp2d_tile(ext, axis, halo, &p)) {
    p.verdict = kLbpHalo;
    return p;
  }
  for (int d = 0; d < 3; d++) p.tiles[d] = ((long long)ext[d] + p.tile[d] - 1) / p.tile[d];      // (of the largest box)
  long long n = 0;
  for (int b = 0; b < B; b++) {
    long long c = 1;
    for (int d = 0; d < 3; d++) c *= ((long long)sizes[3 * b + d] + p.tile[d] - 1) / p.tile[d];
    n += c;
  }
  p.groups = n;
  if (n > kLbpMaxGroups) {
    p.verdict = kLbpGrid;
    return p;
  }
  if (!items) return p;
  long long k = 0;
  for (int b = 0; b < B; b++)
    for (int z = 0; z < sizes[3 * b]; z += p.tile[0])
      for (int y = 0; y < sizes[3 * b + 1]; y += p.tile[1])
        for (int x = 0; x < sizes[3 * b + 2]; x += p.tile[2]) items[k++] = BatchLbpItem{b, z, y, x};
  return p;
}

}  // namespace prad
