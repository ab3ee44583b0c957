// kernels_glszm_zones.h -- what both segment-mode GLSZM models feed: zone statistics, the (level, size) histograms of phase 2
// (float64 [Ng][maxRegion], or [Ng][k] over the k distinct sizes), the ranking of the distinct sizes on the device, the ordered
// zone list.  A kernel is handed parent / rootctl / tinfo for the dense model (zones are the ids with parent[id] == id) and
// nullptr for a label volume (zones are the voxels with labels[i] == i).
#pragma once
#include "prad_runtime.h"

namespace prad {
// stats[0] = max zone size, stats64[0] = zone count.  Also records which zone sizes occur, for the compact fill:
// sizes below PRAD_SMALL_SIZES in a bitmap (LDS per block, OR-ed out once), the few larger ones (at most
// n / PRAD_SMALL_SIZES zones) appended to a list.
#define PRAD_SMALL_SIZES 8192
__global__ void __launch_bounds__(256) glszm_stats_kernel(long long n, const int *__restrict__ labels,
                                                          const unsigned *__restrict__ sizes, int *__restrict__ stats,
                                                          unsigned long long *__restrict__ stats64,
                                                          unsigned *__restrict__ small_bits, int *__restrict__ large_list,
                                                          int large_cap, int *__restrict__ large_count,
                                                          const int *__restrict__ flags,
                                                          const int *__restrict__ parent = nullptr,
                                                          const int *__restrict__ rootctl = nullptr) {
  // parent != nullptr: the dense model (glszm_tile8_kernel) -- entry j < rootctl[0] is a zone root when parent[j] == j and
  // `sizes` is tsize[]; otherwise the zone roots are the voxels with labels[i] == i
  __shared__ unsigned bits[PRAD_SMALL_SIZES / 32];
  __shared__ unsigned smx;
  __shared__ unsigned long long scnt;
  if (flags && flags[0]) return;
  for (int k = threadIdx.x; k < PRAD_SMALL_SIZES / 32; k += blockDim.x) bits[k] = 0u;
  if (threadIdx.x == 0) { smx = 0u; scnt = 0ull; }
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  unsigned mx = 0;
  unsigned long long cnt = 0;
  auto rootsz = [&](unsigned sz) {
    cnt++;
    mx = max(mx, sz);
    if (sz < PRAD_SMALL_SIZES) {
      const unsigned bit = 1u << (sz & 31);
      if (!(bits[sz >> 5] & bit)) atomicOr(bits + (sz >> 5), bit);
    } else {
      const int pos = atomicAdd(large_count, 1);
      if (pos < large_cap) large_list[pos] = (int)sz;
    }
  };
  auto root = [&](long long i) { rootsz(sizes[i]); };
  if (parent) {
    const long long m = rootctl[0], m4 = m >> 2;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < m4; q += stride) {
      const int4 p = reinterpret_cast<const int4 *>(parent)[q];
      const int j = (int)(q << 2);
      if (p.x == j || p.y == j + 1 || p.z == j + 2 || p.w == j + 3) {
        const uint4 z = reinterpret_cast<const uint4 *>(sizes)[q];
        if (p.x == j) rootsz(z.x);
        if (p.y == j + 1) rootsz(z.y);
        if (p.z == j + 2) rootsz(z.z);
        if (p.w == j + 3) rootsz(z.w);
      }
    }
    for (long long j = (m4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride)
      if (parent[j] == (int)j) root(j);
  } else {
    // the scan is a stream over the labels: 16 B per lane and load
    const long long n4 = n >> 2;
    const int4 *lab4 = reinterpret_cast<const int4 *>(labels);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
      const int4 l = lab4[q];
      const long long i = q << 2;
      if (l.x == (int)i) root(i);
      if (l.y == (int)i + 1) root(i + 1);
      if (l.z == (int)i + 2) root(i + 2);
      if (l.w == (int)i + 3) root(i + 3);
    }
    for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
      if (labels[i] == (int)i) root(i);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    cnt += __shfl_xor(cnt, o);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicMax(&smx, mx);
    atomicAdd(&scnt, cnt);
  }
  __syncthreads();
  if (threadIdx.x == 0 && scnt) {
    atomicMax(stats, (int)smx);
    atomicAdd(stats64, scnt);
  }
  for (int k = threadIdx.x; k < PRAD_SMALL_SIZES / 32; k += blockDim.x)
    if (bits[k]) atomicOr(small_bits + k, bits[k]);
}

// column of a zone size in the compact matrix: table lookup below PRAD_SMALL_SIZES, binary search above
__device__ __forceinline__ int glszm_rank(unsigned sz, const int *__restrict__ small_rank, int nsmall,
                                          const int *__restrict__ large_sorted, int nlarge) {
  if (sz < PRAD_SMALL_SIZES) return small_rank[sz];
  int lo = 0, hi = nlarge;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)large_sorted[mid] < sz) lo = mid + 1;
    else hi = mid;
  }
  return (lo < nlarge && (unsigned)large_sorted[lo] == sz) ? nsmall + lo : -1;
}

// Zone counts concentrate on the smallest sizes (noise-like volumes have millions of 1..10-voxel zones), so the
// first RL size columns of every level are accumulated in LDS per block and flushed once; the rest go to HBM.
__global__ void __launch_bounds__(256) glszm_fill_segment_kernel(long long n, const int *__restrict__ labels,
                                                                 const unsigned *__restrict__ sizes,
                                                                 const int *__restrict__ image, int Ng, int maxRegion,
                                                                 int RL, double *__restrict__ out,
                                                                 int *__restrict__ err,
                                                                 const int *__restrict__ parent = nullptr,
                                                                 const int *__restrict__ rootctl = nullptr,
                                                                 const unsigned *__restrict__ tinfo = nullptr) {
  extern __shared__ unsigned fh[];
  for (int k = threadIdx.x; k < Ng * RL; k += blockDim.x) fh[k] = 0u;
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  const unsigned long long idx_max = (unsigned long long)Ng * maxRegion;
  if (parent) n = rootctl[0];            // the dense model: entries of the tile-root list, levels from tinfo[]
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if ((parent ? parent[i] : labels[i]) != (int)i) continue;
    const int gl = parent ? (int)(tinfo[i] >> 16) : image[i];
    const unsigned sz = sizes[i];
    const unsigned long long idx = (unsigned long long)((long long)(gl - 1) * maxRegion + (long long)sz - 1);
    if (gl <= 0 || idx >= idx_max) {  // cmatrices.c:290-291
      *err = 1;
      continue;
    }
    if (gl <= Ng && sz >= 1u && sz <= (unsigned)RL) atomicAdd(fh + (gl - 1) * RL + (sz - 1), 1u);
    else atomicAdd(out + idx, 1.0);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < Ng * RL; k += blockDim.x)
    if (fh[k]) atomicAdd(out + (size_t)(k / RL) * maxRegion + (k % RL), (double)fh[k]);
}

// compact fill (segment mode): the reference's [Ng][maxRegion] layout is almost entirely zero columns when zones are
// large (a smooth 256^3 volume has maxRegion in the millions but only a few thousand distinct sizes -- at most
// sqrt(2 n) since distinct sizes sum to <= n).  The distinct sizes come from glszm_stats_kernel's bookkeeping.
__global__ void __launch_bounds__(256) glszm_fill_compact_kernel(long long n, const int *__restrict__ labels,
                                                                 const unsigned *__restrict__ sizes,
                                                                 const int *__restrict__ image, int Ng, int k, int RL,
                                                                 const int *__restrict__ small_rank, int nsmall,
                                                                 const int *__restrict__ large_sorted, int nlarge,
                                                                 double *__restrict__ out, int *__restrict__ err,
                                                                 const int *__restrict__ parent = nullptr,
                                                                 const int *__restrict__ rootctl = nullptr,
                                                                 const int *__restrict__ meta = nullptr, int kstride = 0,
                                                                 const unsigned *__restrict__ tinfo = nullptr) {
  extern __shared__ unsigned fh[];
  // meta (glszm_rank_kernel: the distinct sizes were ranked on the device, the host does not know k): nsmall, nlarge, k
  // come from there, the rows of `out` are kstride (the capacity) apart; meta[3] != 0: nothing to fill
  if (meta) {
    if (meta[3]) return;
    nsmall = meta[0];
    nlarge = meta[1];
    k = meta[2];
  } else {
    kstride = k;
  }
  // (dense ids: every workgroup takes a contiguous block of at least 4096 of them, the ones left without any return before
  // they touch their 32 KB histogram -- a structured volume has a few hundred thousand ids, noise has millions)
  long long dlo = 0, dhi = 0;
  if (parent) {
    const long long m = rootctl[0];
    const long long per = (max(4096LL, (m + gridDim.x - 1) / gridDim.x) + 3) & ~3LL;
    dlo = (long long)blockIdx.x * per;
    dhi = min(m, dlo + per);
    if (dlo >= dhi) return;
  }
  for (int q = threadIdx.x; q < Ng * RL; q += blockDim.x) fh[q] = 0u;
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  auto rootls = [&](int gl, unsigned sz) {
    const int r = glszm_rank(sz, small_rank, nsmall, large_sorted, nlarge);
    if (gl <= 0 || gl > Ng || r < 0 || r >= k) {
      *err = 1;
      return;
    }
    if (r < RL) atomicAdd(fh + (gl - 1) * RL + r, 1u);
    else atomicAdd(out + (size_t)(gl - 1) * kstride + r, 1.0);
  };
  auto root = [&](long long i) { rootls(parent ? (int)(tinfo[i] >> 16) : image[i], sizes[i]); };
  if (parent) {      // the dense model (glszm_tile8_kernel): `sizes` is tsize[]; four ids per lane and load
    const long long q1 = dhi >> 2;
    for (long long q = (dlo >> 2) + threadIdx.x; q < q1; q += blockDim.x) {
      const int4 p = reinterpret_cast<const int4 *>(parent)[q];
      const int j = (int)(q << 2);
      if (p.x == j || p.y == j + 1 || p.z == j + 2 || p.w == j + 3) {
        const uint4 z = reinterpret_cast<const uint4 *>(sizes)[q], ti = reinterpret_cast<const uint4 *>(tinfo)[q];
        if (p.x == j) rootls((int)(ti.x >> 16), z.x);
        if (p.y == j + 1) rootls((int)(ti.y >> 16), z.y);
        if (p.z == j + 2) rootls((int)(ti.z >> 16), z.z);
        if (p.w == j + 3) rootls((int)(ti.w >> 16), z.w);
      }
    }
    for (long long j = (q1 << 2) + threadIdx.x; j < dhi; j += blockDim.x)
      if (parent[j] == (int)j) root(j);
  } else {
    const long long n4 = n >> 2;
    const int4 *lab4 = reinterpret_cast<const int4 *>(labels);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
      const int4 l = lab4[q];
      const long long i = q << 2;
      if (l.x == (int)i) root(i);
      if (l.y == (int)i + 1) root(i + 1);
      if (l.z == (int)i + 2) root(i + 2);
      if (l.w == (int)i + 3) root(i + 3);
    }
    for (long long i = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
      if (labels[i] == (int)i) root(i);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Ng * RL; q += blockDim.x)
    if (fh[q]) atomicAdd(out + (size_t)(q / RL) * kstride + (q % RL), (double)fh[q]);
}

// ---- the distinct zone sizes ranked ON THE DEVICE (the case pipeline: no host round trip between zones and features) ----
// One workgroup: small sizes from the bitmap (popcount scan), large sizes sorted (bitonic, LDS) and de-duplicated.
// Writes small_rank[PRAD_SMALL_SIZES], large_sorted[nlarge], jvals[k] (the sizes as doubles, ascending: the columns of the
// compact matrix) and meta = {nsmall, nlarge, k, problem}; problem != 0: more large zones than PRAD_RANK_LARGE, more
// distinct sizes than kcap, a zone list beyond the reference's scratch rule (nzones >= 2 Ns: bit 1), irregular levels
// (bit 0) -- the caller then repeats the call on the synchronous route, which reports what the reference reports.
#define PRAD_RANK_LARGE 4096
__global__ void __launch_bounds__(1024) glszm_rank_kernel(const unsigned *__restrict__ small_bits,
                                                          const int *__restrict__ large_list,
                                                          const int *__restrict__ large_count, int large_cap,
                                                          const int *__restrict__ flags,
                                                          const unsigned long long *__restrict__ nzones, long long Ns2,
                                                          int kcap, int *__restrict__ small_rank,
                                                          int *__restrict__ large_sorted, double *__restrict__ jvals,
                                                          int *__restrict__ meta) {
  __shared__ int key[PRAD_RANK_LARGE];
  __shared__ int scan[1024];
  __shared__ int s_nsmall;
  const int t = threadIdx.x;
  int problem = 0;
  if (flags && flags[0]) problem |= 1;
  if ((long long)nzones[0] >= Ns2) problem |= 2;
  // small sizes: word t of the bitmap (PRAD_SMALL_SIZES / 32 = 256 words)
  const int nwords = PRAD_SMALL_SIZES / 32;
  const unsigned w = t < nwords ? small_bits[t] : 0u;
  scan[t] = __popc(w);
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {          // inclusive Hillis-Steele scan
    const int v = t >= o ? scan[t - o] : 0;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  if (t == 1023) s_nsmall = scan[t];
  int base = scan[t] - __popc(w);
  __syncthreads();
  const int nsmall = s_nsmall;
  if (t < nwords) {
    for (int b = 0; b < 32; b++) {
      const int sz = t * 32 + b;
      if (w & (1u << b)) {
        small_rank[sz] = base;
        if (base < kcap) jvals[base] = (double)sz;
        base++;
      } else {
        small_rank[sz] = -1;
      }
    }
  }
  // large sizes
  int nl = large_count[0];
  if (nl > large_cap || nl > PRAD_RANK_LARGE) {
    problem |= 4;
    nl = 0;
  }
  int P = 1;
  while (P < nl) P <<= 1;
  for (int i = t; i < P; i += 1024) key[i] = i < nl ? large_list[i] : 0x7fffffff;
  __syncthreads();
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = t; i < P; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const int a = key[i], b = key[l];
          const bool up = (i & kk) == 0;
          if ((a > b) == up) { key[i] = b; key[l] = a; }
        }
      }
      __syncthreads();
    }
  // unique: element i starts a new value; ranks by a scan over chunks of 1024
  int running = 0;
  for (int c0 = 0; c0 < nl; c0 += 1024) {
    const int i = c0 + t;
    const int first = (i < nl && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
    scan[t] = first;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int v = t >= o ? scan[t - o] : 0;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    if (first) {
      const int r = running + scan[t] - 1;
      large_sorted[r] = key[i];
      if (nsmall + r < kcap) jvals[nsmall + r] = (double)key[i];
    }
    running += scan[1023];
    __syncthreads();
  }
  if (t == 0) {
    if (nsmall + running > kcap) problem |= 4;
    meta[0] = nsmall;
    meta[1] = running;
    meta[2] = nsmall + running;
    meta[3] = problem;
  }
}

// out[16] of the feature block <- verdict (0 = fine): meta[3] of the ranking, the fill's error word
__global__ void glszm_verdict_kernel(const int *__restrict__ meta, const int *__restrict__ err, double *__restrict__ out) {
  out[0] = (double)(meta[3] | (err[0] ? 8 : 0));
}

// ordered zone list (tempData parity): block counts -> scan -> scatter
#define PRAD_ZL_BLOCK 1024
__global__ void __launch_bounds__(256) glszm_root_count_kernel(long long n, const int *__restrict__ labels,
                                                               unsigned *__restrict__ block_counts) {
  __shared__ unsigned s;
  if (threadIdx.x == 0) s = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * PRAD_ZL_BLOCK;
  unsigned c = 0;
  for (int k = threadIdx.x; k < PRAD_ZL_BLOCK; k += 256) {
    const long long i = base + k;
    if (i < n && labels[i] == (int)i) c++;
  }
  if (c) atomicAdd(&s, c);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = s;
}

// single-workgroup exclusive scan (nblocks is at most n/1024 ~ 2M for a 2^31 array)
__global__ void __launch_bounds__(1024) glszm_scan_kernel(long long nblocks, const unsigned *__restrict__ counts,
                                                          unsigned long long *__restrict__ offsets) {
  __shared__ unsigned long long part[1024];
  const long long per = (nblocks + 1023) / 1024;
  const long long lo = (long long)threadIdx.x * per, hi = min(nblocks, lo + per);
  unsigned long long s = 0;
  for (long long i = lo; i < hi; i++) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < 1024; t++) {
      unsigned long long v = part[t];
      part[t] = run;
      run += v;
    }
  }
  __syncthreads();
  unsigned long long run = part[threadIdx.x];
  for (long long i = lo; i < hi; i++) {
    offsets[i] = run;
    run += counts[i];
  }
}

__global__ void __launch_bounds__(64) glszm_root_scatter_kernel(long long n, const int *__restrict__ labels,
                                                                const unsigned *__restrict__ sizes,
                                                                const int *__restrict__ image,
                                                                const unsigned long long *__restrict__ offsets,
                                                                int *__restrict__ pairs) {
  // one wave per 1024-voxel block, walking it 64 voxels at a time so the output order is the index order
  const long long base = (long long)blockIdx.x * PRAD_ZL_BLOCK;
  unsigned long long out = offsets[blockIdx.x];
  const int lane = threadIdx.x;
  for (int k = 0; k < PRAD_ZL_BLOCK; k += 64) {
    const long long i = base + k + lane;
    const bool root = i < n && labels[i] == (int)i;
    const unsigned long long m = __ballot(root);
    if (root) {
      const unsigned long long rank = __popcll(m & ((1ull << lane) - 1ull));
      pairs[(out + rank) * 2] = image[i];
      pairs[(out + rank) * 2 + 1] = (int)sizes[i];
    }
    out += __popcll(m);
  }
}

}  // namespace prad
