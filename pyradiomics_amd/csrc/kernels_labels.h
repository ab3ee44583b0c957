// kernels_labels.h -- label census: voxel count and bounding box of EVERY label of an integer label map in one pass
// (no reference analogue: the reference looks at one label per execute() call, imageoperations.py:407-445 on
// sitk.LabelStatisticsImageFilter).  gfx950 only.
//
// The map is read once, 1 - 4 bytes per voxel; everything else is arranged so that the pass stays bound by that read:
//   - a wave owns whole pieces of x-rows (an ITEM = 64 lanes x V consecutive voxels of one row), so z and y are the same for
//     all of its lanes and only x needs a per-lane range;
//   - label maps are piecewise constant: a wave first asks whether all of its valid lanes hold ONE value.  If so the item is
//     added to a run the wave keeps in registers (label, count, box) and nothing touches a table until the label changes;
//     if not, every lane merges the equal neighbours among its own V voxels and updates the table for each piece;
//   - tier "lds": the table of the workgroup lives in LDS (ds_add / ds_min / ds_max on 32-bit words) while
//     (max_label + 1) * (1 + 2 Nd) words fit in PRAD_CENSUS_LDS_WORDS (48 KiB: three workgroups per CU by LDS), and the rows
//     that received a voxel are merged into the global table with 64-bit vector atomics at the end of the workgroup;
//   - tier "global": above that bound the runs flush straight to the global table, and a mixed item is split by ballot into
//     one piece per label and voxel position, which joins the run like a whole item (no per-lane atomics in global memory).
// Counts are integer atomics: exact and independent of the order of arrival.
#pragma once

#include "prad_runtime.h"

namespace prad {

#define PRAD_CENSUS_THREADS 512
#define PRAD_CENSUS_INFLIGHT 4          // items a wave loads before it looks at the first of them
#define PRAD_CENSUS_LDS_WORDS 12288     // 48 KiB of 32-bit words
#define PRAD_CENSUS_MAX_LABEL 65535

struct CensusGeo {
  int nd;              // 2 or 3
  int nz, ny, nx;      // nz = 1 for a 2-D map
  int max_label;
  int nchunks;         // items per row
  long long items;     // rows * nchunks
  long long per_wave;  // consecutive items per wave
};

// V voxels of element type T as ints; p is aligned to V * sizeof(T)
template <typename T, int V>
__device__ __forceinline__ void census_load(const T *p, int (&a)[V]) {
  if constexpr (V == 1) {
    a[0] = (int)p[0];
  } else if constexpr (sizeof(T) == 1) {
    const unsigned w = *reinterpret_cast<const unsigned *>(p);
    a[0] = (int)(T)(w & 255u);
    a[1] = (int)(T)((w >> 8) & 255u);
    a[2] = (int)(T)((w >> 16) & 255u);
    a[3] = (int)(T)(w >> 24);
  } else if constexpr (sizeof(T) == 2) {
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    a[0] = (int)(T)(w.x & 65535u);
    a[1] = (int)(T)(w.x >> 16);
    a[2] = (int)(T)(w.y & 65535u);
    a[3] = (int)(T)(w.y >> 16);
  } else {
    const int4 w = *reinterpret_cast<const int4 *>(p);
    a[0] = w.x;
    a[1] = w.y;
    a[2] = w.z;
    a[3] = w.w;
  }
}

// one row of a table: count, lo[nd], hi[nd].  32-bit words in LDS (workgroup scope), 64-bit in global memory (agent scope).
template <typename W_>
__device__ __forceinline__ void census_box(W_ *row, int nd, int cnt, int zlo, int zhi, int ylo, int yhi, int xlo, int xhi) {
  constexpr int scope = sizeof(W_) == 4 ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __hip_atomic_fetch_add(&row[0], (W_)cnt, __ATOMIC_RELAXED, scope);
  int k = 1;
  if (nd == 3) __hip_atomic_fetch_min(&row[k++], (W_)zlo, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_min(&row[k++], (W_)ylo, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_min(&row[k++], (W_)xlo, __ATOMIC_RELAXED, scope);
  if (nd == 3) __hip_atomic_fetch_max(&row[k++], (W_)zhi, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_max(&row[k++], (W_)yhi, __ATOMIC_RELAXED, scope);
  __hip_atomic_fetch_max(&row[k++], (W_)xhi, __ATOMIC_RELAXED, scope);
}

// the run a wave keeps in registers: consecutive items that hold one label everywhere (the same values in every lane)
struct CensusRun {
  int label;   // 0 = empty
  int cnt;
  int zlo, zhi, ylo, yhi, xlo, xhi;
  template <typename W_>
  __device__ __forceinline__ void flush(W_ *table, int W, int nd) const {
    census_box(table + (long long)label * W, nd, cnt, zlo, zhi, ylo, yhi, xlo, xhi);
  }
};

// table [max_label + 1][1 + 2 nd]: row 0 zero; an absent label keeps count 0, lo = size, hi = -1
static __global__ void __launch_bounds__(256) census_init_kernel(long long *table, CensusGeo g) {
  const int W = 1 + 2 * g.nd;
  const long long words = (long long)(g.max_label + 1) * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % W);
    long long v = 0;
    if (i >= W && k >= 1) {
      const int d = (k - 1) % g.nd + (3 - g.nd);         // 0 z, 1 y, 2 x
      v = k <= g.nd ? (long long)(d == 0 ? g.nz : (d == 1 ? g.ny : g.nx)) : -1LL;
    }
    table[i] = v;
  }
}

template <typename T, int V, bool LDS>
static __global__ void __launch_bounds__(PRAD_CENSUS_THREADS) label_census_kernel(const T *__restrict__ mask, CensusGeo g,
                                                                                 long long *table) {
  extern __shared__ int census_lds[];
  const int W = 1 + 2 * g.nd;
  const int M = g.max_label;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < (M + 1) * W; i += blockDim.x) {
      const int k = i % W;
      census_lds[i] = k == 0 ? 0 : (k <= g.nd ? 2147483647 : -1);
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long long first = wave * g.per_wave;
  const long long last = first + g.per_wave < g.items ? first + g.per_wave : g.items;
  CensusRun run;
  run.label = 0;

  // adds a piece that holds `label` everywhere to the wave's run (every argument is the same in every lane)
  auto run_add = [&](int label, int n, int z, int y, int xlo, int xhi) {
    if (label != run.label) {
      if (run.label != 0 && lane == 0) {
        if constexpr (LDS) run.flush(census_lds, W, g.nd);
        else run.flush(table, W, g.nd);
      }
      run.label = label;
      run.cnt = 0;
      run.zlo = run.zhi = z;
      run.ylo = run.yhi = y;
      run.xlo = xlo;
      run.xhi = xhi;
    }
    run.cnt += n;
    run.zlo = z < run.zlo ? z : run.zlo;
    run.zhi = z > run.zhi ? z : run.zhi;
    run.ylo = y < run.ylo ? y : run.ylo;
    run.yhi = y > run.yhi ? y : run.yhi;
    run.xlo = xlo < run.xlo ? xlo : run.xlo;
    run.xhi = xhi > run.xhi ? xhi : run.xhi;
  };
  // (z, y, chunk) of the next item, advanced item by item: one division per wave instead of three per item
  int nz_ = 0, ny_ = 0, nc_ = 0;
  if (first < last) {
    const long long r0 = first / g.nchunks;
    nc_ = (int)(first - r0 * g.nchunks);
    nz_ = (int)(r0 / g.ny);
    ny_ = (int)(r0 - (long long)nz_ * g.ny);
  }
  for (long long base = first; base < last; base += PRAD_CENSUS_INFLIGHT) {
    int a[PRAD_CENSUS_INFLIGHT][V];
    int zz[PRAD_CENSUS_INFLIGHT], yy[PRAD_CENSUS_INFLIGHT], xc[PRAD_CENSUS_INFLIGHT];
#pragma unroll
    for (int u = 0; u < PRAD_CENSUS_INFLIGHT; u++) {
      const bool live = base + u < last;                   // the same in every lane
      zz[u] = nz_;
      yy[u] = ny_;
      xc[u] = live ? nc_ * 64 * V : g.nx;
      const int x = xc[u] + lane * V;
#pragma unroll
      for (int j = 0; j < V; j++) a[u][j] = 0;
      if (x < g.nx)                                        // (V == 4: nx is a multiple of 4, the whole lane is inside)
        census_load<T, V>(mask + (((long long)nz_ * g.ny + ny_) * g.nx + x), a[u]);
      if (++nc_ == g.nchunks) {
        nc_ = 0;
        if (++ny_ == g.ny) {
          ny_ = 0;
          ++nz_;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PRAD_CENSUS_INFLIGHT; u++) {
      if (xc[u] >= g.nx) continue;                         // past the end of this wave's items (the same in every lane)
      const int x = xc[u] + lane * V;
      const bool valid = x < g.nx;
      const int z = zz[u], y = yy[u];
      const int head = __builtin_amdgcn_readfirstlane(a[u][0]);      // lane 0 is valid in every live item
      bool same = true;
#pragma unroll
      for (int j = 0; j < V; j++) same = same && a[u][j] == head;
      if (__ballot(valid && !same) == 0ull) {
        // one value in the whole item: extend the wave's run, or start a new one
        if ((unsigned)head - 1u >= (unsigned)M) continue;  // background, negative or above max_label: ignored
        const int n = g.nx - xc[u] < 64 * V ? g.nx - xc[u] : 64 * V;
        run_add(head, n, z, y, xc[u], xc[u] + n - 1);
      } else if constexpr (LDS) {
        // mixed item: every lane merges the equal neighbours among its own voxels, one table update per piece
        if (valid) {
          int cur = a[u][0], start = 0;
#pragma unroll
          for (int j = 1; j <= V; j++) {
            if (j == V || a[u][j < V ? j : 0] != cur) {
              if ((unsigned)cur - 1u < (unsigned)M)
                census_box(census_lds + cur * W, g.nd, j - start, z, z, y, y, x + start, x + j - 1);
              cur = a[u][j < V ? j : 0];
              start = j;
            }
          }
        }
      } else {
        // mixed item, table in global memory: per voxel position j the lanes that hold one label are found by ballot -- x grows
        // with the lane, so the lowest and highest set bit give that label's x range and the bit count its voxels -- and go
        // into the wave's run like a whole item: a label that fills part of a row costs no atomic until another one follows
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int v = a[u][j];
          unsigned long long todo = __ballot(valid && (unsigned)v - 1u < (unsigned)M);
          while (todo) {
            const int lv = __shfl(v, (int)__ffsll((long long)todo) - 1);
            const unsigned long long m = __ballot(valid && v == lv);
            run_add(lv, (int)__popcll(m), z, y, xc[u] + ((int)__ffsll((long long)m) - 1) * V + j,
                    xc[u] + (63 - (int)__clzll((long long)m)) * V + j);
            todo &= ~m;
          }
        }
      }
    }
  }
  if (run.label != 0 && lane == 0) {
    if constexpr (LDS) run.flush(census_lds, W, g.nd);
    else run.flush(table, W, g.nd);
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int v = 1 + (int)threadIdx.x; v <= M; v += blockDim.x) {
      const int *r = census_lds + v * W;
      if (r[0] == 0) continue;
      long long *t = table + (long long)v * W;
      __hip_atomic_fetch_add(&t[0], (long long)r[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int k = 1; k <= g.nd; k++) {
        __hip_atomic_fetch_min(&t[k], (long long)r[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&t[k + g.nd], (long long)r[k + g.nd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// largest element of an integer array (sizes the census table when the caller names no max_label): 16-byte loads over the
// aligned body, the few elements in front of and behind it by the first workgroup, one atomic per workgroup
template <typename T>
static __global__ void __launch_bounds__(256) mask_max_kernel(const T *__restrict__ p, long long n, long long *out) {
  __shared__ int block_max;
  if (threadIdx.x == 0) block_max = -2147483647 - 1;
  __syncthreads();
  constexpr int E = 16 / (int)sizeof(T);
  const unsigned long long addr = (unsigned long long)p;
  long long head = (long long)(((16 - (addr & 15)) & 15) / sizeof(T));
  head = head < n ? head : n;
  const long long nvec = (n - head) / E;
  int m = -2147483647 - 1;
  const uint4 *q = reinterpret_cast<const uint4 *>(p + head);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long long)gridDim.x * blockDim.x) {
    const uint4 w = q[i];
    const T *e = reinterpret_cast<const T *>(&w);
#pragma unroll
    for (int j = 0; j < E; j++) m = (int)e[j] > m ? (int)e[j] : m;
  }
  if (blockIdx.x == 0) {
    for (long long i = threadIdx.x; i < head; i += blockDim.x) m = (int)p[i] > m ? (int)p[i] : m;
    for (long long i = head + nvec * E + threadIdx.x; i < n; i += blockDim.x) m = (int)p[i] > m ? (int)p[i] : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(m, off);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_max(&block_max, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_max(out, (long long)block_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static __global__ void set_ll_kernel(long long *p, long long v) { *p = v; }

}  // namespace prad
