// kernels_box.h -- the bounding box of a kernel (voxel mode) or of the whole array, and raster walks inside it: inline device helpers
#pragma once
#include "prad_runtime.h"

namespace prad {

__device__ __forceinline__ void kernel_box(const Geo &g, const VoxMode &vm, int v, int *lo, int *hi) {
  for (int d = 0; d < g.nd; d++) {
    if (!vm.voxels) {
      lo[d] = 0;
      hi[d] = g.size[d] - 1;
    } else {
      int c = vm.voxels[(long long)d * vm.nvox + v];
      if (d == vm.f2d) {
        lo[d] = hi[d] = c;  // _cmatrices.c:1127-1128
      } else {
        lo[d] = max(c - vm.radius, 0);
        hi[d] = min(c + vm.radius, g.size[d] - 1);
      }
    }
  }
}

// decode box-local raster index k into coordinates; false if k is beyond the box
__device__ __forceinline__ bool box_decode(const Geo &g, const int *lo, const int *hi, long long k, int *c,
                                           long long *offset) {
  long long off = 0;
  for (int d = g.nd - 1; d >= 0; d--) {
    int ext = hi[d] - lo[d] + 1;
    if (ext <= 0) return false;
    int q = (int)(k % ext);
    k /= ext;
    c[d] = lo[d] + q;
    off += (long long)c[d] * g.stride[d];
  }
  *offset = off;
  return k == 0;
}

__device__ __forceinline__ long long box_step(const Geo &g, const int *lo, const int *hi, const int *c,
                                              const int *ang, int sign) {
  long long off = 0;
  for (int d = 0; d < g.nd; d++) {
    int q = c[d] + sign * ang[d];
    if (q < lo[d] || q > hi[d]) return -1;
    off += (long long)q * g.stride[d];
  }
  return off;
}

}  // namespace prad
