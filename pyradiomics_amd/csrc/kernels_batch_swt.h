// kernels_batch_swt.h -- the wavelet sub-bands of MANY small boxes in ONE launch (gfx950): the level-1, undecimated, periodised
// 3-D transform of swt3_fused_kernel (kernels_filters.h) on the batch layout of kernels_batch_firstorder.h, with the wrapped
// sample the reference appends to every odd axis (imageoperations.py:914-919) folded into the index arithmetic.
//
// batch_swt_kernel<F, TIN>.  ROI b is the box [Nz][Ny][Nx] at element `off` of the packed image (TIN: int16 / int32 / float32 /
// float64, widened to float64 when staged: exact); band k of it goes to out + k * band_stride + off, in the box's own shape,
// k = (bx * 2 + by) * 2 + bz as swt_level1_dev numbers the bands for axes (2, 1, 0).
//   periods   an axis of length N is periodic with period P = N + (N & 1): position N of an odd axis reads sample 0.  Only
//             positions below N are computed for storing: no padded copy, no crop.
//   work      one workgroup per ITEM of a host-built table (batch_swt_plan below): a (y, x) tile of one ROI and a z range of
//             it.  Work is divided by output, not by ROI: a 40^3 box next to 300 boxes of 6^3 becomes 45 workgroups.
//   scheme    that of swt3_fused_kernel: the workgroup streams its tile along z; each input plane of the tile with its F - 1
//             halo rows and columns is staged in LDS, the x pass leaves lo / hi rows in LDS, every lane runs the y pass for its
//             own (y, x) and keeps the four y-bands of the last F planes in registers, from which the z pass produces the eight
//             outputs of a finished plane.  A z range re-stages F - 1 warm-up planes.
//   tiles     (TY, TX) = (32, 8), (16, 16) or (8, 32), chosen per ROI by the planner (fewest tiles, then the smallest staged
//             area): the record carries log2 TX, the workgroup branches once (uniformly) into the body compiled for its shape;
//             the LDS is dynamic, sized by the host for the largest shape of the three (PRAD_BSWT_LDS_DOUBLES(F)).
//   sums      every 1-D sum starts from 0.0 and takes the taps in ascending k, float64 throughout, and EVERY term is one
//             fma(tap, v, sum) -- the first one too, fma(tap, v, 0.0).  That is what the device compiler makes of the
//             __dadd_rn(s, __dmul_rn(tap, v)) of swt3_fused_kernel under its default contraction (84 v_fma_f64 / v_fmac_f64 and
//             not one v_mul_f64 or v_add_f64 in swt3_fused_kernel<6, float>, and so in all twelve instantiations); here the
//             fma is spelled out, so the sub-bands are the single route's bits by construction, not by the optimiser's leave
//             (tests/test_gpu_batch_wavelet.py compares the bytes).
//   indices   offsets into the batch are 64-bit; inside a box 32-bit indices suffice (the host declines boxes above 2^31 - 1
//             voxels).  No atomics, no memset; nothing outside the boxes of the native ROIs is written.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; 256 lanes per workgroup):
//   F  TIN (all four alike)  VGPRs  AGPRs  SGPRs  scratch  LDS (dynamic: the largest shape of F)  waves per SIMD
//   6                          72      0    102        0  10 816 B (1 352 doubles, shape 8 x 32)         7
//   4                          55      0     93        0   8 976 B (1 122 doubles, shape 8 x 32)         8
//   2                          36      0     81        0   7 392 B (  924 doubles, shape 32 x 8)         8
// Registers bound the residency (7 workgroups per compute unit at F = 6, where the LDS would allow 14).  Filters of 8, 10 and
// 12 taps are not instantiated.
#pragma once
#include "prad_runtime.h"

namespace prad {

#ifndef PRAD_MAX_TAPS
#define PRAD_MAX_TAPS 32      // (kernels_filters.h: the longest filter the single route takes)
#endif
#define PRAD_BSWT_THREADS 256
#define PRAD_BSWT_MAX_F 6
// z planes of the shortest range a box is cut into, and the number of items up to which boxes are cut at all
#ifndef PRAD_BSWT_MIN_CZ
#define PRAD_BSWT_MIN_CZ 8
#endif
#ifndef PRAD_BSWT_TARGET_ITEMS
#define PRAD_BSWT_TARGET_ITEMS 1024      // (-DPRAD_BSWT_TARGET_ITEMS=2048: the variant of profiles/batch_wavelet_measurements.md)
#endif
// doubles of LDS of the tile shape with log2 TX = L: S0 [HY][HX + 1], then two [HY][TX + 1]
#define PRAD_BSWT_SHAPE_DOUBLES(F, L) \
  ((((256 >> (L)) + (F)-1) * ((1 << (L)) + (F))) + 2 * (((256 >> (L)) + (F)-1) * ((1 << (L)) + 1)))
#define PRAD_BSWT_MAX2(a, b) ((a) > (b) ? (a) : (b))
#define PRAD_BSWT_LDS_DOUBLES(F) \
  PRAD_BSWT_MAX2(PRAD_BSWT_SHAPE_DOUBLES(F, 3), PRAD_BSWT_MAX2(PRAD_BSWT_SHAPE_DOUBLES(F, 4), PRAD_BSWT_SHAPE_DOUBLES(F, 5)))

struct BatchSwtTaps {
  double lo[PRAD_BSWT_MAX_F];
  double hi[PRAD_BSWT_MAX_F];
};

struct BatchSwtRoi {
  long long off;      // first element of the box in the packed image and in every band
  int nz, ny, nx;
  int ltx;            // log2 TX of the ROI's tile shape: 3, 4 or 5
  int pad[2];
};
static_assert(sizeof(BatchSwtRoi) == 32, "BatchSwtRoi is uploaded as an array of 32-byte records");

// one workgroup: the outputs [z0, z1) x [y0, y1) x [x0, x1) of ROI roi; y1 - y0 <= TY, x1 - x0 <= TX (the ranges are clipped to
// the box).  Also the row of the table prad_batch_swt_plan hands out (8 ints).
struct BatchSwtItem {
  int roi, z0, z1, y0, y1, x0, x1, tx;
};
static_assert(sizeof(BatchSwtItem) == 32, "BatchSwtItem is 8 ints");

// ---- the planner: host only, pure -------------------------------------------------------------------------------------------
inline int bswt_padded(int n) { return n + (n & 1); }
inline bool bswt_flen_native(int flen) { return flen == 2 || flen == 4 || flen == 6; }
// a ROI is native when every padded extent holds the filter (the condition of the fused single kernel) and its voxels can be
// indexed with 32 bits
inline bool bswt_roi_native(const int *size, int flen) {
  if (!bswt_flen_native(flen)) return false;
  if ((long long)size[0] * size[1] * size[2] > 2147483647LL) return false;
  return bswt_padded(size[0]) >= flen && bswt_padded(size[1]) >= flen && bswt_padded(size[2]) >= flen;
}
// log2 TX of the tile shape of a box: the fewest tiles, then the smallest staged plane (TY + F - 1) (TX + F - 1), then the
// widest rows
inline int bswt_tile_shape(int ny, int nx, int flen) {
  int best = 5;
  long long best_tiles = -1, best_area = 0;
  for (int l = 5; l >= 3; l--) {
    const int tx = 1 << l, ty = 256 >> l;
    const long long tiles = (long long)((ny + ty - 1) / ty) * ((nx + tx - 1) / tx);
    const long long area = (long long)(ty + flen - 1) * (tx + flen - 1);
    if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && area < best_area)) {
      best = l;
      best_tiles = tiles;
      best_area = area;
    }
  }
  return best;
}
inline long long bswt_tiles(const int *size, int ltx) {
  const int tx = 1 << ltx, ty = 256 >> ltx;
  return (long long)((size[1] + ty - 1) / ty) * ((size[2] + tx - 1) / tx);
}
// The chunk length CZ of a call: a box of nz planes is cut into ceil(nz / CZ) z ranges of equal length (the last may be
// shorter).  A range costs its length + F - 1 plane steps, so cutting only ever adds work; it pays while the launch has fewer
// items than the GPU holds workgroups at once (4 per compute unit on 256 units: PRAD_BSWT_TARGET_ITEMS).  CZ is the largest
// length at which the native ROIs make that many items, and never below PRAD_BSWT_MIN_CZ.
inline int bswt_chunk_length(const int *sizes, int B, int flen) {
  int top = PRAD_BSWT_MIN_CZ;
  for (int b = 0; b < B; b++)
    if (bswt_roi_native(sizes + 3 * b, flen)) top = sizes[3 * b] > top ? sizes[3 * b] : top;
  auto items_at = [&](int cz) {
    long long n = 0;
    for (int b = 0; b < B; b++) {
      const int *s = sizes + 3 * b;
      if (bswt_roi_native(s, flen)) n += bswt_tiles(s, bswt_tile_shape(s[1], s[2], flen)) * ((s[0] + cz - 1) / cz);
    }
    return n;
  };
  if (items_at(top) >= PRAD_BSWT_TARGET_ITEMS) return top;
  // items_at does not grow with cz: bisect the largest cz in [MIN_CZ, top] that reaches the target
  int lo = PRAD_BSWT_MIN_CZ, hi = top;
  if (items_at(lo) < PRAD_BSWT_TARGET_ITEMS) return lo;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (items_at(mid) >= PRAD_BSWT_TARGET_ITEMS) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// verdict int [B]: 0 native, 8 the single route; *n_items = the workgroups of the launch; items (may be NULL) receives them and
// ltx (may be NULL, int [B]) the tile shape of every native ROI.  Sizes have been checked (>= 1).
inline void batch_swt_plan(const int *sizes, int B, int flen, int *verdict, long long *n_items, BatchSwtItem *items, int *ltx) {
  const int cz = bswt_chunk_length(sizes, B, flen);
  long long n = 0;
  for (int b = 0; b < B; b++) {
    const int *s = sizes + 3 * b;
    const bool native = bswt_roi_native(s, flen);
    if (verdict) verdict[b] = native ? 0 : 8;
    if (!native) continue;
    const int l = bswt_tile_shape(s[1], s[2], flen), tx = 1 << l, ty = 256 >> l;
    if (ltx) ltx[b] = l;
    const int nzc = (s[0] + cz - 1) / cz, len = (s[0] + nzc - 1) / nzc;
    for (int z0 = 0; z0 < s[0]; z0 += len)
      for (int y0 = 0; y0 < s[1]; y0 += ty)
        for (int x0 = 0; x0 < s[2]; x0 += tx) {
          if (items) {
            BatchSwtItem &it = items[n];
            it.roi = b;
            it.z0 = z0;
            it.z1 = z0 + len < s[0] ? z0 + len : s[0];
            it.y0 = y0;
            it.y1 = y0 + ty < s[1] ? y0 + ty : s[1];
            it.x0 = x0;
            it.x1 = x0 + tx < s[2] ? x0 + tx : s[2];
            it.tx = tx;
          }
          n++;
        }
  }
  *n_items = n;
}

#if defined(__HIPCC__)
// position p of an axis of length n and period pn = n + (n & 1), p in (-pn, ...): the sample it reads
__device__ __forceinline__ int bswt_wrap(int p, int n, int pn) {
  p = p < 0 ? p + pn : p;
  p = p >= pn ? p - pn : p;
  p = p >= pn ? p % pn : p;      // (ragged last tiles reach further than one period; their outputs are not stored)
  return p >= n ? 0 : p;         // (p == n on an odd axis: the wrapped sample)
}

template <int F, int LTX, typename TIN>
__device__ __forceinline__ void batch_swt_body(const TIN *__restrict__ x, const BatchSwtRoi &R, const BatchSwtItem &I,
                                               const BatchSwtTaps &T, double *__restrict__ out, long long band_stride,
                                               double *__restrict__ lds) {
  constexpr int TX = 1 << LTX, TY = 256 >> LTX;
  constexpr int HY = TY + F - 1, HX = TX + F - 1, LOH = F - 1 - F / 2;
  constexpr int P0 = HX + 1, PA = TX + 1;      // row pitches
  double *S0 = lds, *A = lds + HY * P0, *D = A + HY * PA;
  const int Nz = R.nz, Ny = R.ny, Nx = R.nx, Pz = Nz + (Nz & 1), Py = Ny + (Ny & 1), Px = Nx + (Nx & 1);
  const int tid = threadIdx.x, tx = tid & (TX - 1), ty = tid >> LTX;
  const int x0 = I.x0, y0 = I.y0, zc0 = I.z0, zc1 = I.z1;
  const bool mine = (y0 + ty) < I.y1 && (x0 + tx) < I.x1;
  const TIN *__restrict__ box = x + R.off;
  double *__restrict__ o = out + R.off;
  double r[4][F];                      // the y-bands (aa, ad, da, dd) of the last F planes at this lane's (y, x); [0] = newest
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int k = 0; k < F; k++) r[b][k] = 0.0;
  const int steps = (zc1 - zc0) + F - 1;
  for (int s = 0; s < steps; s++) {
    const int zp = bswt_wrap(zc0 - LOH + s, Nz, Pz);
    const TIN *__restrict__ plane = box + (long long)zp * Ny * Nx;
    for (int e = tid; e < HY * HX; e += PRAD_BSWT_THREADS) {
      const int iy = e / HX, ix = e - iy * HX;
      const int gy = bswt_wrap(y0 - LOH + iy, Ny, Py), gx = bswt_wrap(x0 - LOH + ix, Nx, Px);
      S0[iy * P0 + ix] = (double)plane[gy * Nx + gx];
    }
    __syncthreads();
    for (int e = tid; e < HY * TX; e += PRAD_BSWT_THREADS) {
      const int iy = e >> LTX, ox = e & (TX - 1);
      double sl = 0.0, sh = 0.0;
#pragma unroll
      for (int k = 0; k < F; k++) {
        const double v = S0[iy * P0 + ox + F - 1 - k];
        sl = __builtin_fma(T.lo[k], v, sl);
        sh = __builtin_fma(T.hi[k], v, sh);
      }
      A[iy * PA + ox] = sl;
      D[iy * PA + ox] = sh;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
      for (int k = F - 1; k >= 1; k--) r[b][k] = r[b][k - 1];
    {
      double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
#pragma unroll
      for (int k = 0; k < F; k++) {
        const double va = A[(ty + F - 1 - k) * PA + tx], vd = D[(ty + F - 1 - k) * PA + tx];
        aa = __builtin_fma(T.lo[k], va, aa);
        ad = __builtin_fma(T.hi[k], va, ad);
        da = __builtin_fma(T.lo[k], vd, da);
        dd = __builtin_fma(T.hi[k], vd, dd);
      }
      r[0][0] = aa; r[1][0] = ad; r[2][0] = da; r[3][0] = dd;
    }
    if (s >= F - 1 && mine) {
      const int oz = zc0 + s - (F - 1);
      const long long vi = ((long long)oz * Ny + (y0 + ty)) * Nx + (x0 + tx);
#pragma unroll
      for (int b = 0; b < 4; b++) {
        double sl = 0.0, sh = 0.0;
#pragma unroll
        for (int k = 0; k < F; k++) {
          sl = __builtin_fma(T.lo[k], r[b][k], sl);
          sh = __builtin_fma(T.hi[k], r[b][k], sh);
        }
        o[(long long)(2 * b) * band_stride + vi] = sl;
        o[(long long)(2 * b + 1) * band_stride + vi] = sh;
      }
    }
  }
}

template <int F, typename TIN>
__global__ void __launch_bounds__(PRAD_BSWT_THREADS)
batch_swt_kernel(const TIN *__restrict__ x, const BatchSwtRoi *__restrict__ rois, const BatchSwtItem *__restrict__ items,
                 BatchSwtTaps T, double *__restrict__ out, long long band_stride) {
  extern __shared__ double bswt_lds[];
  const BatchSwtItem I = items[blockIdx.x];
  const BatchSwtRoi R = rois[I.roi];
  switch (R.ltx) {      // (uniform: one shape per workgroup)
    case 3: batch_swt_body<F, 3, TIN>(x, R, I, T, out, band_stride, bswt_lds); break;
    case 4: batch_swt_body<F, 4, TIN>(x, R, I, T, out, band_stride, bswt_lds); break;
    default: batch_swt_body<F, 5, TIN>(x, R, I, T, out, band_stride, bswt_lds); break;
  }
}
#endif  // __HIPCC__

}  // namespace prad
