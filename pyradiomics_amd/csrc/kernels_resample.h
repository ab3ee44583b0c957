// kernels_resample.h -- the resampling step in front of the path (radiomics/imageoperations.py:448-612, ITK's
// ResampleImageFilter with BSplineInterpolateImageFunction / NearestNeighborInterpolateImageFunction), for an output grid
// whose axes are those of the input (image and mask share one grid): output voxel o along axis d sits at the continuous
// input index start[d] + o * step[d].
//   to_f64_kernel              image -> float64 coefficient volume
//   bspline_prefilter_kernel   BSplineDecompositionImageFilter along one axis, in place, one lane per line: gain, causal
//                              initialisation over the 1e-10 horizon (or the exact mirror sum for short lines), causal
//                              and anti-causal recursion with the pole sqrt(3) - 2 (the line body is bspline_prefilter_line,
//                              which kernels_batch_resample.h runs on the lines of many boxes in one launch)
//   resample_kernel            one thread per output voxel: cubic B-spline weights on the mirrored 4^Nd support (or
//                              linear / nearest), inside-buffer test, clamp + truncating cast to the pixel type
// Multiplications and additions are kept unfused and in the order of pyradiomics_amd.imageoperations.resampleImage
// (x contraction innermost), whose results the reference's `_resampling` golden vectors pin: both produce the same bits.
#pragma once
#include "prad_runtime.h"

namespace prad {

template <typename T>
__global__ void to_f64_kernel(const T *__restrict__ in, long long n, double *__restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = (double)in[i];
}

// one line of N samples, `st` doubles apart, filtered in place (N == 1 leaves it alone); shared with kernels_batch_resample.h
__device__ __forceinline__ void bspline_prefilter_line(double *p, int N, long long st, int horizon) {
#pragma clang fp contract(off)
  if (N == 1) return;
  const double z = sqrt(3.0) - 2.0;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int n = 0; n < N; n++) p[n * st] *= gain;
  if (horizon < N) {
    double zn = z, acc = p[0];
    for (int n = 1; n < horizon; n++) {
      acc += zn * p[n * st];
      zn *= z;
    }
    p[0] = acc;
  } else {
    const double iz = 1.0 / z;
    double z2n = pow(z, (double)(N - 1)), zn = z;
    double acc = p[0] + z2n * p[(long long)(N - 1) * st];
    z2n *= z2n * iz;
    for (int n = 1; n < N - 1; n++) {
      acc += (zn + z2n) * p[n * st];
      zn *= z;
      z2n *= iz;
    }
    p[0] = acc / (1.0 - zn * zn);
  }
  double prev = p[0];
  for (int n = 1; n < N; n++) {
    const double v = p[n * st] + z * prev;
    p[n * st] = v;
    prev = v;
  }
  double last = (z / (z * z - 1.0)) * (z * p[(long long)(N - 2) * st] + p[(long long)(N - 1) * st]);
  p[(long long)(N - 1) * st] = last;
  for (int n = N - 2; n >= 0; n--) {
    const double v = z * (last - p[n * st]);
    p[n * st] = v;
    last = v;
  }
}

// c viewed as [outer][N][inner]  (static: the header is included by two translation units)
static __global__ void __launch_bounds__(256) bspline_prefilter_kernel(double *__restrict__ c, long long outer, int N,
                                                                       long long inner, int horizon) {
  const long long lines = outer * inner;
  const long long line = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (line >= lines || N == 1) return;
  bspline_prefilter_line(c + (line / inner) * N * inner + (line % inner), N, inner, horizon);
}

struct ResampleGeo {
  int nd;
  int in[3], out[3];          // sizes, numpy order (z, y, x) right-aligned in 3 slots (leading 1s)
  double start[3], step[3];
};

__device__ __forceinline__ int mirror_index(long long i, int N) {
  if (N == 1) return 0;
  const long long L2 = 2LL * N - 2;
  long long r = i < 0 ? -i - L2 * ((-i) / L2) : i - L2 * (i / L2);
  if (r >= N) r = L2 - r;
  return (int)r;
}
__device__ __forceinline__ void bspline_weights(double pos, long long *base, double w[4]) {
#pragma clang fp contract(off)
  const double fl = floor(pos);
  *base = (long long)fl - 1;
  const double t = pos - (double)(*base + 1);
  w[3] = (1.0 / 6.0) * t * t * t;
  w[0] = (1.0 / 6.0) + 0.5 * t * (t - 1.0) - w[3];
  w[2] = t + w[0] - 2.0 * w[3];
  w[1] = 1.0 - w[0] - w[2] - w[3];
}

// interp: 0 nearest (value copied from `src`), 1 linear (from src), 3 cubic B-spline (from the coefficients `coef`)
template <typename T>
__global__ void __launch_bounds__(256) resample_kernel(const T *__restrict__ src, const double *__restrict__ coef,
                                                       ResampleGeo g, int interp, int is_integer, double tmin,
                                                       double tmax, T *__restrict__ out) {
#pragma clang fp contract(off)
  const long long nout = (long long)g.out[0] * g.out[1] * g.out[2];
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long sy = g.in[2], sz = (long long)g.in[1] * g.in[2];
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < nout; o += stride) {
    const int ox = (int)(o % g.out[2]), oy = (int)((o / g.out[2]) % g.out[1]), oz = (int)(o / ((long long)g.out[2] * g.out[1]));
    const double px = g.start[2] + (double)ox * g.step[2], py = g.start[1] + (double)oy * g.step[1],
                 pz = g.start[0] + (double)oz * g.step[0];
    const bool inside = px >= -0.5 && px < g.in[2] - 0.5 && py >= -0.5 && py < g.in[1] - 0.5 && pz >= -0.5 &&
                        pz < g.in[0] - 0.5;
    if (!inside) {
      out[o] = (T)0;
      continue;
    }
    double val;
    if (interp == 0) {
      const int ix = min(max((int)floor(px + 0.5), 0), g.in[2] - 1), iy = min(max((int)floor(py + 0.5), 0), g.in[1] - 1),
                iz = min(max((int)floor(pz + 0.5), 0), g.in[0] - 1);
      out[o] = src[iz * sz + iy * sy + ix];
      continue;
    } else if (interp == 1) {
      const long long bx = (long long)floor(px), by = (long long)floor(py), bz = (long long)floor(pz);
      const double fx = px - (double)bx, fy = py - (double)by, fz = pz - (double)bz;
      auto cl = [](long long i, int N) { return (int)min(max(i, 0LL), (long long)N - 1); };
      double zs[2];
      for (int kz = 0; kz < 2; kz++) {
        double ys[2];
        for (int ky = 0; ky < 2; ky++) {
          const long long row = cl(bz + kz, g.in[0]) * sz + cl(by + ky, g.in[1]) * sy;
          ys[ky] = (double)src[row + cl(bx, g.in[2])] * (1 - fx) + (double)src[row + cl(bx + 1, g.in[2])] * fx;
        }
        zs[kz] = ys[0] * (1 - fy) + ys[1] * fy;
      }
      val = zs[0] * (1 - fz) + zs[1] * fz;
    } else {
      long long bx, by, bz;
      double wx[4], wy[4], wz[4];
      bspline_weights(px, &bx, wx);
      bspline_weights(py, &by, wy);
      bspline_weights(pz, &bz, wz);
      int ix[4], iy[4], iz[4];
      for (int k = 0; k < 4; k++) {
        ix[k] = mirror_index(bx + k, g.in[2]);
        iy[k] = mirror_index(by + k, g.in[1]);
        iz[k] = mirror_index(bz + k, g.in[0]);
      }
      double vz = 0;
      for (int kz = 0; kz < 4; kz++) {
        double vy = 0;
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
    out[o] = (T)val;
  }
}

}  // namespace prad
