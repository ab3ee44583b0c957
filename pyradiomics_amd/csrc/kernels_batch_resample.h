// kernels_batch_resample.h -- the resampling step of the batched small-ROI route (gfx950): B boxes in the packed batch layout
// (kernels_batch_firstorder.h), each with a grid of its own, are resampled in at most THREE launches whatever B is.  Per box
// the arithmetic is that of kernels_resample.h applied to the box as if it were the whole image -- the same device functions,
// the same order, unfused -- so a box gives the bits prad_resample_dev gives for it.
//
//   batch_mask_boxes_kernel          one workgroup per ROI: the uint8 mask (non-zero = ROI) reduced to lo z/y/x, hi z/y/x and
//                                    the voxel count, seven ints per ROI (an empty mask: lo = the sizes, hi = -1, count 0).
//   batch_bspline_prefilter_kernel   one workgroup of 256 lanes per ROI interpolated with the cubic B-spline: the image is
//                                    widened into the float64 coefficient scratch, then the x, y and z passes of
//                                    bspline_prefilter_line run one after another (ITK's order), one lane per line, lanes
//                                    looping over the lines, __syncthreads() between the passes.  A workgroup hands data only
//                                    to itself, through global memory: the barrier's workgroup-scope fence is all it needs.
//   batch_resample_kernel            work divided by OUTPUT voxels: the native ROIs form a line of W = sum nout items, item
//                                    w[b] + e being output voxel e of ROI b, workgroup c takes [c * CHUNK, (c + 1) * CHUNK)
//                                    and a lane bisects w[] between first[c] and first[c + 1] (host-built), as
//                                    batch_gather_kernel does: an up-sampled 30^3 box spreads over many workgroups.  Per
//                                    output voxel: resample_kernel's body; the mask of the same ROI is resampled
//                                    nearest-neighbour (uint8 -> uint8) on the same grid in the same launch.  Coefficients
//                                    are read straight from global memory / L2.
// Index arithmetic is 64-bit; the split of an item into (z, y, x) uses 32-bit divisions when the ROI has fewer than 2^32
// output voxels.
#pragma once
#include "kernels_resample.h"

namespace prad {

#define PRAD_BRES_THREADS 256
#define PRAD_BRES_PER_LANE 4
#define PRAD_BRES_CHUNK (PRAD_BRES_THREADS * PRAD_BRES_PER_LANE)

struct MaskBoxRoi {
  long long off;     // first element of the box in the packed mask
  int nz, ny, nx;
  int pad;
};
static_assert(sizeof(MaskBoxRoi) == 24, "MaskBoxRoi is uploaded as an array of 24-byte records");

struct BatchResampleRoi {
  long long in_off;     // first element of the box in the packed image / mask
  long long out_off;    // first element of the ROI in the packed outputs
  long long coef_off;   // first double of the box in the coefficient scratch (B-spline ROIs)
  long long w;          // first work item of the ROI (prefix sum of the output voxels)
  long long nout;
  double start[3], step[3];     // z, y, x
  int in[3], out[3];
  int interp;                   // 0 nearest, 1 linear, 3 cubic B-spline
  int pad;
};
static_assert(sizeof(BatchResampleRoi) == 120, "BatchResampleRoi is uploaded as an array of 120-byte records");

__global__ void __launch_bounds__(PRAD_BRES_THREADS)
batch_mask_boxes_kernel(const unsigned char *__restrict__ mask, const MaskBoxRoi *__restrict__ rois, int *__restrict__ boxes) {
  __shared__ int red[7][PRAD_BRES_THREADS];
  const MaskBoxRoi r = rois[blockIdx.x];
  const long long n = (long long)r.nz * r.ny * r.nx, plane = (long long)r.ny * r.nx;
  const unsigned char *m = mask + r.off;
  int lo_z = r.nz, lo_y = r.ny, lo_x = r.nx, hi_z = -1, hi_y = -1, hi_x = -1, count = 0;
  for (long long e = threadIdx.x; e < n; e += PRAD_BRES_THREADS) {
    if (m[e] == 0) continue;
    int z, y, x;
    if (n <= 0xffffffffLL) {
      const unsigned e32 = (unsigned)e, q = e32 / (unsigned)plane, rem = e32 - q * (unsigned)plane, y32 = rem / (unsigned)r.nx;
      z = (int)q;
      y = (int)y32;
      x = (int)(rem - y32 * (unsigned)r.nx);
    } else {
      const long long q = e / plane, rem = e - q * plane, yy = rem / r.nx;
      z = (int)q;
      y = (int)yy;
      x = (int)(rem - yy * r.nx);
    }
    lo_z = min(lo_z, z);
    lo_y = min(lo_y, y);
    lo_x = min(lo_x, x);
    hi_z = max(hi_z, z);
    hi_y = max(hi_y, y);
    hi_x = max(hi_x, x);
    count++;
  }
  const int t = threadIdx.x;
  red[0][t] = lo_z;
  red[1][t] = lo_y;
  red[2][t] = lo_x;
  red[3][t] = hi_z;
  red[4][t] = hi_y;
  red[5][t] = hi_x;
  red[6][t] = count;
  __syncthreads();
  for (int half = PRAD_BRES_THREADS / 2; half > 0; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (int k = 0; k < 3; k++) red[k][t] = min(red[k][t], red[k][t + half]);
#pragma unroll
      for (int k = 3; k < 6; k++) red[k][t] = max(red[k][t], red[k][t + half]);
      red[6][t] += red[6][t + half];
    }
    __syncthreads();
  }
  if (t < 7) boxes[7 * (long long)blockIdx.x + t] = red[t][0];
}

// ROI bs[blockIdx.x] of the record table: image -> coefficients, x, y, z pass
template <typename T>
__global__ void __launch_bounds__(PRAD_BRES_THREADS)
batch_bspline_prefilter_kernel(const T *__restrict__ image, const BatchResampleRoi *__restrict__ rois, const int *__restrict__ bs,
                               double *coef, int horizon) {
  const BatchResampleRoi *r = rois + bs[blockIdx.x];
  const int nz = r->in[0], ny = r->in[1], nx = r->in[2];
  const long long plane = (long long)ny * nx, n = plane * nz;
  const T *src = image + r->in_off;
  double *c = coef + r->coef_off;
  for (long long e = threadIdx.x; e < n; e += PRAD_BRES_THREADS) c[e] = (double)src[e];
  __syncthreads();
  if (nx > 1)
    for (long long line = threadIdx.x; line < (long long)nz * ny; line += PRAD_BRES_THREADS)
      bspline_prefilter_line(c + line * nx, nx, 1, horizon);
  __syncthreads();
  if (ny > 1)
    for (long long line = threadIdx.x; line < (long long)nz * nx; line += PRAD_BRES_THREADS)
      bspline_prefilter_line(c + (line / nx) * plane + (line % nx), ny, nx, horizon);
  __syncthreads();
  if (nz > 1)
    for (long long line = threadIdx.x; line < plane; line += PRAD_BRES_THREADS) bspline_prefilter_line(c + line, nz, plane, horizon);
}

template <typename T>
__global__ void __launch_bounds__(PRAD_BRES_THREADS)
batch_resample_kernel(const T *__restrict__ image, const unsigned char *__restrict__ mask, const double *__restrict__ coefs,
                      const BatchResampleRoi *__restrict__ rois, const int *__restrict__ first, long long total,
                      T *__restrict__ out, unsigned char *__restrict__ out_mask) {
#pragma clang fp contract(off)
  constexpr bool is_integer = std::is_integral<T>::value;
  constexpr double tmin = std::is_same<T, short>::value ? -32768.0 : -2147483648.0;
  constexpr double tmax = std::is_same<T, short>::value ? 32767.0 : 2147483647.0;
  const long long chunk = blockIdx.x;
  const int b_lo = first[chunk], b_hi = first[chunk + 1];
#pragma unroll 1
  for (int k = 0; k < PRAD_BRES_PER_LANE; k++) {
    const long long item = chunk * PRAD_BRES_CHUNK + (long long)k * PRAD_BRES_THREADS + threadIdx.x;
    if (item >= total) break;
    int a = b_lo, z = b_hi;          // the last ROI of [b_lo, b_hi] with w <= item
    while (a < z) {
      const int m = (a + z + 1) >> 1;
      if (rois[m].w <= item) a = m;
      else z = m - 1;
    }
    const BatchResampleRoi *r = rois + a;
    const long long e = item - r->w;
    const int n0 = r->in[0], n1 = r->in[1], n2 = r->in[2], o1 = r->out[1], o2 = r->out[2];
    int ox, oy, oz;
    if (r->nout <= 0xffffffffLL) {
      const unsigned plane = (unsigned)o1 * (unsigned)o2, e32 = (unsigned)e;
      const unsigned q = e32 / plane, rem = e32 - q * plane, y32 = rem / (unsigned)o2;
      oz = (int)q;
      oy = (int)y32;
      ox = (int)(rem - y32 * (unsigned)o2);
    } else {
      const long long plane = (long long)o1 * o2, q = e / plane, rem = e - q * plane, yy = rem / o2;
      oz = (int)q;
      oy = (int)yy;
      ox = (int)(rem - yy * o2);
    }
    const long long sy = n2, sz = (long long)n1 * n2;
    const long long to = r->out_off + e;
    const double px = r->start[2] + (double)ox * r->step[2], py = r->start[1] + (double)oy * r->step[1],
                 pz = r->start[0] + (double)oz * r->step[0];
    const bool inside = px >= -0.5 && px < n2 - 0.5 && py >= -0.5 && py < n1 - 0.5 && pz >= -0.5 && pz < n0 - 0.5;
    if (!inside) {
      out[to] = (T)0;
      if (out_mask) out_mask[to] = 0;
      continue;
    }
    const int interp = r->interp;
    const T *src = image + r->in_off;
    if (out_mask || interp == 0) {
      const int ix = min(max((int)floor(px + 0.5), 0), n2 - 1), iy = min(max((int)floor(py + 0.5), 0), n1 - 1),
                iz = min(max((int)floor(pz + 0.5), 0), n0 - 1);
      const long long from = iz * sz + iy * sy + ix;
      if (out_mask) out_mask[to] = mask[r->in_off + from];
      if (interp == 0) {
        out[to] = src[from];
        continue;
      }
    }
    double val;
    if (interp == 1) {
      const long long bx = (long long)floor(px), by = (long long)floor(py), bz = (long long)floor(pz);
      const double fx = px - (double)bx, fy = py - (double)by, fz = pz - (double)bz;
      auto cl = [](long long i, int N) { return (int)min(max(i, 0LL), (long long)N - 1); };
      double zs[2];
#pragma unroll
      for (int kz = 0; kz < 2; kz++) {
        double ys[2];
#pragma unroll
        for (int ky = 0; ky < 2; ky++) {
          const long long row = cl(bz + kz, n0) * sz + cl(by + ky, n1) * sy;
          ys[ky] = (double)src[row + cl(bx, n2)] * (1 - fx) + (double)src[row + cl(bx + 1, n2)] * fx;
        }
        zs[kz] = ys[0] * (1 - fy) + ys[1] * fy;
      }
      val = zs[0] * (1 - fz) + zs[1] * fz;
    } else {
      const double *coef = coefs + r->coef_off;
      long long bx, by, bz;
      double wx[4], wy[4], wz[4];
      bspline_weights(px, &bx, wx);
      bspline_weights(py, &by, wy);
      bspline_weights(pz, &bz, wz);
      int ix[4], iy[4], iz[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        ix[q] = mirror_index(bx + q, n2);
        iy[q] = mirror_index(by + q, n1);
        iz[q] = mirror_index(bz + q, n0);
      }
      double vz = 0;
#pragma unroll
      for (int kz = 0; kz < 4; kz++) {
        double vy = 0;
#pragma unroll
        for (int ky = 0; ky < 4; ky++) {
          const double *row = coef + iz[kz] * sz + iy[ky] * sy;
          double vx = row[ix[0]] * wx[0];
          vx = vx + row[ix[1]] * wx[1];
          vx = vx + row[ix[2]] * wx[2];
          vx = vx + row[ix[3]] * wx[3];
          vy = ky == 0 ? vx * wy[0] : vy + vx * wy[ky];
        }
        vz = kz == 0 ? vy * wz[0] : vz + vy * wz[kz];
      }
      val = vz;
    }
    if (is_integer) {                    // ResampleImageFilter::CastPixelWithBoundsChecking: clamp, then a C cast
      val = fmin(fmax(val, tmin), tmax);
      val = trunc(val);
    }
    out[to] = (T)val;
  }
}

}  // namespace prad
