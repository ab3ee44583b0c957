// kernels_glszm_labels.h -- GLSZM zones (cmatrices.c:94-297) as a LABEL VOLUME: the int32 kernels of segment mode.
//
// label[i] = i (masked) | -1, unions by atomicMin on the larger root (the returned old value keeps the structure consistent
// when views are stale), flatten, count; the root of a zone is its smallest linear index = the voxel where the reference's
// raster scan discovers the zone, so listing roots in index order reproduces the reference's tempData order exactly.
//   label-volume route (any Nd, any angle set):  glszm_init_kernel, glszm_merge_kernel, glszm_flatten_count_kernel
//   int32 tiles (Nd <= 3, unit offsets):         glszm_tile_kernel, one of glszm_border_full_kernel<1|2> / glszm_border_kernel,
//                                                glszm_rootsum_kernel
// Which route a call takes, the tile and Offsets3: prad_glszm_plan.h.  lds_find / lds_union also serve kernels_glszm_dense.h.
#pragma once
#include "prad_runtime.h"
#include "prad_glszm_plan.h"

namespace prad {

__global__ void glszm_init_kernel(const uint8_t *__restrict__ mask, long long n, int *__restrict__ labels,
                                  unsigned *__restrict__ sizes) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    labels[i] = mask[i] ? (int)i : -1;
    sizes[i] = 0;
  }
}

// find with path halving.  Labels only ever decrease towards the root, so a racing / stale view at worst repeats
// a hop; writing the grandparent is always a valid shortcut (it is an ancestor).
__device__ __forceinline__ int uf_find(int *labels, int i) {
  int p = __builtin_nontemporal_load(labels + i);
  while (p != i) {
    const int g = __builtin_nontemporal_load(labels + p);
    if (g != p) labels[i] = g;
    i = p;
    p = g;
  }
  return i;
}

__device__ __forceinline__ void uf_union(int *labels, int a, int b) {
  while (true) {
    a = uf_find(labels, a);
    b = uf_find(labels, b);
    if (a == b) return;
    if (a < b) { int t = a; a = b; b = t; }
    const int old = atomicMin(labels + a, b);
    if (old == a) return;  // a was a root and now points to b
    a = old;               // a had already been linked elsewhere: join that set with b's
  }
}

__global__ void __launch_bounds__(256) glszm_merge_kernel(Geo g, const int *__restrict__ angles, int Na,
                                                          const int *__restrict__ image,
                                                          const uint8_t *__restrict__ mask,
                                                          int *__restrict__ labels) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    if (!mask[i]) continue;
    int c[PRAD_MAX_ND];
    long long rem = i;
    for (int d = 0; d < g.nd; d++) {
      c[d] = (int)(rem / g.stride[d]);
      rem -= (long long)c[d] * g.stride[d];
    }
    const int gl = image[i];
    for (int a = 0; a < Na; a++) {
      long long j = 0;
      bool in = true;
      for (int d = 0; d < g.nd; d++) {
        const int q = c[d] + angles[a * g.nd + d];
        if (q < 0 || q >= g.size[d]) { in = false; break; }
        j += (long long)q * g.stride[d];
      }
      if (!in || j >= i) continue;  // only backward neighbours: each adjacent pair is united once
      if (mask[j] && image[j] == gl) uf_union(labels, (int)i, (int)j);
    }
  }
}

// ---- tiled variant (Nd <= 3): zones are first labelled inside 4 x 8 x 64 tiles entirely in LDS, then only voxel
// pairs that straddle a tile boundary are united in HBM.  Most unions (and all of their retries on large zones)
// never leave the CU; the global forest starts from one root per (zone, tile) instead of one per voxel.
// `lab` is a __shared__ array.  The loads are typed as LDS loads: through a generic `volatile int *` the compiler emits
// flat_load ... sc0 sc1 (system scope, the flat path's latency) for every hop of the pointer chase -- 64 M of them per
// 512^3 volume in glszm_tile8_kernel, 2/3 of its time (profiles/r04_probes.md section 11).
typedef __attribute__((address_space(3))) int lds_int_t;
__device__ __forceinline__ int lds_find(int *lab, int i) {
  volatile lds_int_t *l = (volatile lds_int_t *)lab;
  int p;
  while ((p = l[i]) != i) i = p;
  return i;
}
__device__ __forceinline__ void lds_union(int *lab, int a, int b) {
  while (true) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) { int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);
    if (old == a) return;
    a = old;
  }
}

// mode: 0 = any offset list, 1 = the full 26-neighbourhood (13 backward offsets), 2 = the full in-plane
// 8-neighbourhood (4 backward offsets, dz = 0)
__global__ void __launch_bounds__(256) glszm_tile_kernel(Offsets3 A, int mode, const int *__restrict__ image,
                                                         const uint8_t *__restrict__ mask, int Nz, int Ny, int Nx,
                                                         int *__restrict__ labels, unsigned *__restrict__ sizes) {
  __shared__ int img[PRAD_TVOX];
  __shared__ int lab[PRAD_TVOX];
  __shared__ uint8_t msk[PRAD_TVOX];
  const int tx = (Nx + PRAD_TX - 1) / PRAD_TX, ty = (Ny + PRAD_TY - 1) / PRAD_TY;
  const int bz = blockIdx.x / (ty * tx), br = blockIdx.x % (ty * tx);
  const int z0 = bz * PRAD_TZ, y0 = (br / tx) * PRAD_TY, x0 = (br % tx) * PRAD_TX;
  for (int k = threadIdx.x; k < PRAD_TVOX; k += blockDim.x) {
    const int lx = k % PRAD_TX, ly = (k / PRAD_TX) % PRAD_TY, lz = k / (PRAD_TX * PRAD_TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    const bool in = z < Nz && y < Ny && x < Nx;
    const long long gi = ((long long)z * Ny + y) * Nx + x;
    const bool m = in && mask[gi] != 0;
    msk[k] = m;
    img[k] = m ? image[gi] : 0;
    lab[k] = k;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < PRAD_TVOX; k += blockDim.x) {
    if (!msk[k]) continue;
    const int lx = k % PRAD_TX, ly = (k / PRAD_TX) % PRAD_TY, lz = k / (PRAD_TX * PRAD_TY);
    const int gl = img[k];
    // in-tile index of the neighbour at (dz, dy, dx) if it lies in the tile and continues the zone, else -1
    auto same = [&](int dz, int dy, int dx) -> int {
      const int qz = lz + dz, qy = ly + dy, qx = lx + dx;
      if ((unsigned)qz >= PRAD_TZ || (unsigned)qy >= PRAD_TY || (unsigned)qx >= PRAD_TX) return -1;
      const int j = (qz * PRAD_TY + qy) * PRAD_TX + qx;
      return (msk[j] && img[j] == gl) ? j : -1;
    };
    if (mode == 0) {
      for (int a = 0; a < A.na; a++) {
        const int j = same(A.o[a][0], A.o[a][1], A.o[a][2]);
        if (j >= 0) lds_union(lab, k, j);
      }
      continue;
    }
    // Full 8- / 26-neighbourhoods: a neighbour that is itself adjacent (within its plane) to one already united
    // with k belongs to the same zone through that plane's own unions, so its union is redundant.  On smooth data
    // this leaves ~2 unions per voxel instead of ~10.
    const int b = same(0, -1, 0);                    // in-plane: b is adjacent to a, c and d
    if (b >= 0) lds_union(lab, k, b);
    else {
      const int a = same(0, -1, -1), c = same(0, -1, 1), d = same(0, 0, -1);
      if (c >= 0) lds_union(lab, k, c);
      if (a >= 0) lds_union(lab, k, a);              // a and d are adjacent to each other
      else if (d >= 0) lds_union(lab, k, d);
    }
    if (mode == 1) {                                 // plane above: its centre is adjacent to the other eight
      const int m = same(-1, 0, 0);
      if (m >= 0) lds_union(lab, k, m);
      else {
        const int e1 = same(-1, -1, 0), e2 = same(-1, 1, 0), e3 = same(-1, 0, -1), e4 = same(-1, 0, 1);
        if (e1 >= 0) lds_union(lab, k, e1);
        if (e2 >= 0) lds_union(lab, k, e2);
        if (e3 >= 0) lds_union(lab, k, e3);
        if (e4 >= 0) lds_union(lab, k, e4);
        int q;                                       // a corner is adjacent to the two edges next to it
        if (e1 < 0 && e3 < 0 && (q = same(-1, -1, -1)) >= 0) lds_union(lab, k, q);
        if (e1 < 0 && e4 < 0 && (q = same(-1, -1, 1)) >= 0) lds_union(lab, k, q);
        if (e2 < 0 && e3 < 0 && (q = same(-1, 1, -1)) >= 0) lds_union(lab, k, q);
        if (e2 < 0 && e4 < 0 && (q = same(-1, 1, 1)) >= 0) lds_union(lab, k, q);
      }
    }
  }
  __syncthreads();
  // flatten inside the tile and count each local component: img[] is reused for the counts (its levels are no
  // longer needed), runs of equal roots among the lanes of a wave issue one LDS atomic
  int root[PRAD_TVOX / 256];
#pragma unroll
  for (int q = 0; q < PRAD_TVOX / 256; q++) {
    const int k = threadIdx.x + q * 256;
    root[q] = msk[k] ? lds_find(lab, k) : -1;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < PRAD_TVOX; k += blockDim.x) img[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < PRAD_TVOX / 256; q++) {
    const int r = root[q];
    int left = __shfl_up(r, 1);
    if (lane == 0) left = -2;
    const unsigned long long B = __ballot(r != left || lane == 0);
    if (r >= 0 && r != left) {
      const unsigned long long above = lane == 63 ? 0ull : (B >> (lane + 1));
      atomicAdd((unsigned *)img + r, (unsigned)(above ? __ffsll((long long)above) : 64 - lane));
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PRAD_TVOX / 256; q++) {
    const int k = threadIdx.x + q * 256;
    const int lx = k % PRAD_TX, ly = (k / PRAD_TX) % PRAD_TY, lz = k / (PRAD_TX * PRAD_TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    if (z >= Nz || y >= Ny || x >= Nx) continue;
    const long long gi = ((long long)z * Ny + y) * Nx + x;
    const int r = root[q];
    if (r < 0) { labels[gi] = -1; sizes[gi] = 0; continue; }
    const int rx = r % PRAD_TX, ry = (r / PRAD_TX) % PRAD_TY, rz = r / (PRAD_TX * PRAD_TY);
    labels[gi] = (int)(((long long)(z0 + rz) * Ny + (y0 + ry)) * Nx + (x0 + rx));   // local raster order == global order
    sizes[gi] = r == k ? (unsigned)img[k] : 0u;     // voxels of the local component, kept at its (tile) root
  }
}

// unions across tile boundaries only.  The union runs between the two tile roots (labels[] of a non-root voxel is
// one hop from its tile root and is never rewritten), and a lane whose (root, root) pair repeats its left
// neighbour's -- the usual case along a face shared by two large components -- skips the union altogether.
__global__ void __launch_bounds__(256) glszm_border_kernel(Offsets3 A, const int *__restrict__ image,
                                                           const uint8_t *__restrict__ mask, int Nz, int Ny, int Nx,
                                                           int *__restrict__ labels) {
  // One wave per row (z, y).  Rows on a z- or y-face of their tile are scanned completely; in all other rows only
  // the two x-faces of every tile (x mod 64 in {0, 63}) can have a backward neighbour in another tile, so the wave
  // visits just those.  No per-voxel index decoding: z, y are wave-uniform, x comes from the lane.
  const int lane = threadIdx.x & 63;
  const long long nrows = (long long)Nz * Ny;
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int xtiles = (Nx + PRAD_TX - 1) / PRAD_TX;
  for (long long row = wave0; row < nrows; row += nwaves) {
    const int z = (int)(row / Ny), y = (int)(row - (long long)z * Ny);
    const bool row_edge = (z % PRAD_TZ == 0) || (y % PRAD_TY == 0) || (y % PRAD_TY == PRAD_TY - 1);
    const int count = row_edge ? Nx : 2 * xtiles;            // candidates in this row
    const long long rbase = row * Nx;
    for (int c0 = 0; c0 < count; c0 += 64) {
      const int c = c0 + lane;
      int x = -1;
      if (c < count) x = row_edge ? c : (c >> 1) * PRAD_TX + ((c & 1) ? PRAD_TX - 1 : 0);
      int gl = 0, li = -1;
      if (x >= 0 && x < Nx && mask[rbase + x]) {
        gl = image[rbase + x];
        li = labels[rbase + x];
      }
      if (__ballot(li >= 0) == 0ull) continue;
      for (int a = 0; a < A.na; a++) {
        int lj = -1;
        if (li >= 0) {
          const int qz = z + A.o[a][0], qy = y + A.o[a][1], qx = x + A.o[a][2];
          const bool in = (unsigned)qz < (unsigned)Nz && (unsigned)qy < (unsigned)Ny && (unsigned)qx < (unsigned)Nx;
          const bool same_tile = qz / PRAD_TZ == z / PRAD_TZ && qy / PRAD_TY == y / PRAD_TY && qx / PRAD_TX == x / PRAD_TX;
          if (in && !same_tile) {
            const long long j = ((long long)qz * Ny + qy) * Nx + qx;
            if (mask[j] && image[j] == gl) lj = labels[j];
          }
        }
        const int pi = __shfl_up(li, 1), pj = __shfl_up(lj, 1);
        if (lj >= 0 && !(lane > 0 && pi == li && pj == lj)) uf_union(labels, li, lj);
      }
    }
  }
}

// The same scan for the full 26- (MODE 1) / in-plane 8-neighbourhood (MODE 2) with the redundancy rules of the tile
// kernel applied to GLOBAL sameness: a backward neighbour whose own (earlier) unions already tie it to a neighbour we
// unite with is skipped -- and so are its loads.  By induction over raster order every adjacent same-level pair still
// ends up connected: each voxel is united with one representative of every cluster of mutually adjacent backward
// neighbours, and the members of a cluster are adjacent voxels that precede it.  Pairs inside one tile are left to
// the tile kernel (which applies the rules to in-tile sameness and therefore performs a superset of them).
template <int MODE>
__global__ void __launch_bounds__(256) glszm_border_full_kernel(const int *__restrict__ image,
                                                                const uint8_t *__restrict__ mask, int Nz, int Ny,
                                                                int Nx, int *__restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const long long nrows = (long long)Nz * Ny;
  const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  const int xtiles = (Nx + PRAD_TX - 1) / PRAD_TX;
  for (long long row = wave0; row < nrows; row += nwaves) {
    const int z = (int)(row / Ny), y = (int)(row - (long long)z * Ny);
    const bool row_edge = (MODE == 1 && z % PRAD_TZ == 0) || (y % PRAD_TY == 0) || (MODE == 1 && y % PRAD_TY == PRAD_TY - 1);
    const int count = row_edge ? Nx : 2 * xtiles;
    const long long rbase = row * Nx;
    for (int c0 = 0; c0 < count; c0 += 64) {
      const int c = c0 + lane;
      int x = -1;
      if (c < count) x = row_edge ? c : (c >> 1) * PRAD_TX + ((c & 1) ? PRAD_TX - 1 : 0);
      int gl = 0, li = -1;
      if (x >= 0 && x < Nx && mask[rbase + x]) {
        gl = image[rbase + x];
        li = labels[rbase + x];
      }
      if (__ballot(li >= 0) == 0ull) continue;
      // linear index of the neighbour if it continues the zone, else -1 (only evaluated for live lanes)
      auto same = [&](int dz, int dy, int dx) -> long long {
        const int qz = z + dz, qy = y + dy, qx = x + dx;
        if ((unsigned)qz >= (unsigned)Nz || (unsigned)qy >= (unsigned)Ny || (unsigned)qx >= (unsigned)Nx) return -1;
        const long long j = ((long long)qz * Ny + qy) * Nx + qx;
        return (mask[j] && image[j] == gl) ? j : -1;
      };
      // unite across the tile boundary; every lane of the wave takes part in the shuffle
      auto pair = [&](long long j, int dz, int dy, int dx) {
        int lj = -1;
        if (j >= 0) {
          const int qz = z + dz, qy = y + dy, qx = x + dx;
          const bool same_tile = qz / PRAD_TZ == z / PRAD_TZ && qy / PRAD_TY == y / PRAD_TY && qx / PRAD_TX == x / PRAD_TX;
          if (!same_tile) lj = labels[j];
        }
        const int pi = __shfl_up(li, 1), pj = __shfl_up(lj, 1);
        if (lj >= 0 && !(lane > 0 && pi == li && pj == lj)) uf_union(labels, li, lj);
      };
      const bool live = li >= 0;
      const long long jb = live ? same(0, -1, 0) : -1;
      pair(jb, 0, -1, 0);
      const bool nb = live && jb < 0;
      const long long jc = nb ? same(0, -1, 1) : -1;
      pair(jc, 0, -1, 1);
      const long long ja = nb ? same(0, -1, -1) : -1;
      pair(ja, 0, -1, -1);
      const long long jd = (nb && ja < 0) ? same(0, 0, -1) : -1;
      pair(jd, 0, 0, -1);
      if (MODE == 1) {
        const long long jm = live ? same(-1, 0, 0) : -1;
        pair(jm, -1, 0, 0);
        const bool nm = live && jm < 0;
        const long long e1 = nm ? same(-1, -1, 0) : -1, e2 = nm ? same(-1, 1, 0) : -1;
        const long long e3 = nm ? same(-1, 0, -1) : -1, e4 = nm ? same(-1, 0, 1) : -1;
        pair(e1, -1, -1, 0);
        pair(e2, -1, 1, 0);
        pair(e3, -1, 0, -1);
        pair(e4, -1, 0, 1);
        pair((nm && e1 < 0 && e3 < 0) ? same(-1, -1, -1) : -1, -1, -1, -1);
        pair((nm && e1 < 0 && e4 < 0) ? same(-1, -1, 1) : -1, -1, -1, 1);
        pair((nm && e2 < 0 && e3 < 0) ? same(-1, 1, -1) : -1, -1, 1, -1);
        pair((nm && e2 < 0 && e4 < 0) ? same(-1, 1, 1) : -1, -1, 1, 1);
      }
    }
  }
}

#define PRAD_RS_SLOTS 1024             // LDS hash table of the two root-sum kernels
// int32 tile path: sizes[] holds the voxel count of every tile-local component at its tile root; fold the counts of
// tile roots that were linked elsewhere into their global root.  One find per (zone, tile) instead of per voxel.
// A zone that spans thousands of tiles would otherwise receive thousands of atomics on one address, so every block
// owns a CONTIGUOUS slab of voxels and first combines contributions to the same root in an LDS hash table.
#define PRAD_RS_CHUNK (64 * 256)       // voxels per block (256^3: 1024 blocks; with 65536 the kernel ran 256 blocks, 3x slower)
__global__ void __launch_bounds__(256) glszm_rootsum_kernel(long long n, int *__restrict__ labels,
                                                            unsigned *__restrict__ sizes) {
  __shared__ int hkey[PRAD_RS_SLOTS];
  __shared__ unsigned hval[PRAD_RS_SLOTS];
  const long long lo = (long long)blockIdx.x * PRAD_RS_CHUNK, hi = min(n, lo + PRAD_RS_CHUNK);
  if (lo >= hi) return;
  for (int k = threadIdx.x; k < PRAD_RS_SLOTS; k += blockDim.x) {
    hkey[k] = -1;
    hval[k] = 0u;
  }
  __syncthreads();
  for (long long i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    const unsigned sz = sizes[i];
    if (sz == 0u) continue;
    const int l = labels[i];
    if (l == (int)i) continue;
    const int r = uf_find(labels, l);
    labels[i] = r;
    unsigned slot = ((unsigned)r * 2654435761u) >> 22;          // 10 bits
    bool done = false;
    for (int probe = 0; probe < 8 && !done; probe++, slot = (slot + 1) & (PRAD_RS_SLOTS - 1)) {
      const int old = atomicCAS(hkey + slot, -1, r);
      if (old == -1 || old == r) {
        atomicAdd(hval + slot, sz);
        done = true;
      }
    }
    if (!done) atomicAdd(sizes + r, sz);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < PRAD_RS_SLOTS; k += blockDim.x)
    if (hkey[k] >= 0 && hval[k]) atomicAdd(sizes + hkey[k], hval[k]);
}

__global__ void __launch_bounds__(256) glszm_flatten_count_kernel(long long n, int *__restrict__ labels,
                                                                   unsigned *__restrict__ sizes) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  const long long nround = ((n + stride - 1) / stride) * stride;  // keep whole waves in the loop for the shuffles
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nround; i += stride) {
    int r = -1;
    if (i < n) {
      const int l = labels[i];
      if (l >= 0) {
        r = l;
        int p;
        while ((p = labels[r]) != r) r = p;
        if (r != l) labels[i] = r;
      }
    }
    int left = __shfl_up(r, 1);
    if (lane == 0) left = -2;
    const bool head = (r >= 0) && (r != left);
    const bool brk = (r != left) || lane == 0;          // a run (of any value) starts here
    const unsigned long long B = __ballot(brk);
    if (head) {
      const unsigned long long above = lane == 63 ? 0ull : (B >> (lane + 1));
      const int len = above ? __ffsll((long long)above) : 64 - lane;  // distance to the next run start
      atomicAdd(sizes + r, (unsigned)len);
    }
  }
}

}  // namespace prad
