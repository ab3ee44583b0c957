// kernels_glszm_voxel.h -- GLSZM in voxel mode (many small boxes): one lane per kernel runs the reference's raster-order
// flood fill (cmatrices.c:94-297) inside its box with a private visited map / stack (interleaved [slot][kernel] so
// neighbouring lanes touch neighbouring addresses); the mask itself is never modified, which replaces the reference's
// processedStack restore (cmatrices.c:264-272).
#pragma once
#include "kernels_box.h"

namespace prad {
__global__ void __launch_bounds__(64) glszm_voxel_kernel(Geo g, VoxMode vm, const int *__restrict__ image,
                                                         const uint8_t *__restrict__ mask,
                                                         const int *__restrict__ angles, int Na,
                                                         uint8_t *__restrict__ visited, int *__restrict__ stack,
                                                         int *__restrict__ zones, int *__restrict__ zone_count,
                                                         int *__restrict__ stats,
                                                         unsigned long long *__restrict__ stats64, int Ns_eff) {
  // (one wave per workgroup: the wave's maximum / zone count are combined in LDS and lane 0 -- active whenever any lane of
  // the wave is -- issues the two global atomics; one pair per CENTRE on these two words serialises in L2)
  __shared__ int smx;
  __shared__ unsigned long long snz;
  if (threadIdx.x == 0) { smx = 0; snz = 0ull; }
  __syncthreads();
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= vm.nvox) return;
  const long long NV = vm.nvox;
  int lo[PRAD_MAX_ND], hi[PRAD_MAX_ND], ext[PRAD_MAX_ND], c[PRAD_MAX_ND];
  kernel_box(g, vm, v, lo, hi);
  long long total = 1;
  for (int d = 0; d < g.nd; d++) {
    ext[d] = hi[d] - lo[d] + 1;
    total *= ext[d];
  }
  for (long long k = 0; k < total; k++) visited[k * NV + v] = 0;
  int nz = 0, mx = 0, nproc = 0;
  for (long long k = 0; k < total; k++) {
    if (visited[k * NV + v]) continue;
    long long i;
    box_decode(g, lo, hi, k, c, &i);
    if (!mask[i]) continue;
    if (nz >= 2 * Ns_eff) { stats[1] = 1; break; }  // cmatrices.c:245 (tempData full)
    const int gl = image[i];
    int region = 0;
    long long top = 0;
    stack[(top++) * NV + v] = (int)k;
    visited[k * NV + v] = 1;
    while (top > 0) {
      const long long kk = stack[(--top) * NV + v];
      region++;
      nproc++;
      long long ii;
      box_decode(g, lo, hi, kk, c, &ii);
      for (int a = 0; a < Na; a++) {
        const int *ang = angles + a * g.nd;
        long long j = 0, kj = 0;
        bool in = true;
        for (int d = 0; d < g.nd; d++) {
          const int q = c[d] + ang[d];
          if (q < lo[d] || q > hi[d]) { in = false; break; }
          j += (long long)q * g.stride[d];
          kj = kj * ext[d] + (q - lo[d]);
        }
        if (!in || visited[kj * NV + v] || !mask[j] || image[j] != gl) continue;
        visited[kj * NV + v] = 1;
        stack[(top++) * NV + v] = (int)kj;
      }
    }
    zones[((long long)nz * 2) * NV + v] = gl;
    zones[((long long)nz * 2 + 1) * NV + v] = region;
    nz++;
    mx = max(mx, region);
  }
  if (nproc > Ns_eff || nz >= 2 * Ns_eff) stats[1] = 1;  // cmatrices.c:174,226 (processedStack) and :274
  zone_count[v] = nz;
  if (nz) {
    atomicMax(&smx, mx);
    atomicAdd(&snz, (unsigned long long)nz);
  }
  __syncthreads();
  if (threadIdx.x == 0 && snz) {
    atomicMax(stats, smx);
    atomicAdd(stats64, snz);
  }
}

__global__ void glszm_fill_voxel_kernel(int nvox, long long boxmax, const int *__restrict__ zones,
                                        const int *__restrict__ zone_count, int Ng, int maxRegion,
                                        double *__restrict__ out, int *__restrict__ err) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long z = gid / nvox;
  const int v = (int)(gid % nvox);
  if (z >= boxmax || z >= zone_count[v]) return;
  const int gl = zones[(z * 2) * nvox + v], sz = zones[(z * 2 + 1) * nvox + v];
  const unsigned long long idx_max = (unsigned long long)Ng * maxRegion;
  const unsigned long long idx = (unsigned long long)((long long)(gl - 1) * maxRegion + (long long)sz - 1);
  if (gl <= 0 || idx >= idx_max) {
    *err = 1;
    return;
  }
  atomicAdd(out + (size_t)v * idx_max + idx, 1.0);
}

__global__ void glszm_gather_zones_kernel(int nvox, int v, int count, const int *__restrict__ zones,
                                          int *__restrict__ pairs) {
  const int z = blockIdx.x * blockDim.x + threadIdx.x;
  if (z >= count) return;
  pairs[z * 2] = zones[((long long)z * 2) * nvox + v];
  pairs[z * 2 + 1] = zones[((long long)z * 2 + 1) * nvox + v];
}

}  // namespace prad
