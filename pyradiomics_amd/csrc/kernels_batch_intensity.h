// kernels_batch_intensity.h -- the intensity transforms (Square, SquareRoot, Logarithm, Exponential) and the Gradient magnitude
// of MANY small boxes in at most TWO launches (gfx950), on the batch layout of kernels_batch_firstorder.h: ROI b is the box
// [nz][ny][nx] at element `off` of the packed image (TIN: int16 / int32 / float32 / float64, widened to float64: exact).
//
// batch_intensity_consts_kernel<TIN>   launch 1, one workgroup per ROI, any number of voxels (nothing is kept in LDS but four
//   partial maxima).  top = max |x| in float64 -- the value is widened BEFORE fabs, so int16 -32768 gives 32768 and int32 -2^31
//   gives 2^31 --, a wave butterfly (wave_reduce.h) followed by four words of LDS; fmax drops NaN, so a float box is also
//   scanned for values that are not finite.  One lane writes the verdict (0 native, PRAD_BINT_ZERO top == 0: the formulas of
//   the reference divide by zero, PRAD_BINT_NONFINITE a NaN or an infinity) and the constants of the ROI, with the operations of
//   filters.py in their order: c_sq = 1 / sqrt(top), top, s_log = top / log(top + 1), k_exp = log(top) / top.  (The reference
//   divides by max |sign(x) log(|x| + 1)|; log is monotone, so that maximum is log(top + 1).)
// batch_intensity_kernel<TIN>          launch 2, work divided by output elements as in kernels_batch_gather.h: the batch is a
//   line of W = sum n work items, item w[b] + e being element e of ROI b; workgroup c takes the items of row c of a host-built
//   table (batch_intensity_plan: 1024 consecutive items and the first and last ROI they touch; a lane bisects w[] between the
//   two).  Lane t takes the items t, t + 256, t + 512, t + 768 of the chunk: consecutive lanes load consecutive x of one box
//   row and store consecutive elements of every output row.  x is loaded once for all pointwise types:
//     square       (c_sq x) (c_sq x)                        squareroot   sign(x) sqrt(|x| top)        (sign(0) = 0)
//     logarithm    (sign(x) log(|x| + 1)) s_log             exponential  exp(k_exp x)
//   float64 [rows][row_stride], one row per requested type in the order above.  Gradient (float32, one row): per axis z, y, x of
//   extent > 1, d = 0.5 (x[i + 1] - x[i - 1]) with the neighbour indices clamped to the box, d = d * inv[axis], acc = acc + d d;
//   sqrt(acc) rounded once to float32.  inv is 1 / spacing rounded on the HOST (1 without gradientUseSpacing): dividing a device
//   tensor by a host number is, in torch, the multiplication with that reciprocal, and the single route
//   (filters.getGradientImage) is what every box has to equal bit for bit.
//   Contraction is off in both kernels (#pragma clang fp contract(off)): no product is fused into a sum, every operation is
//   the correctly rounded one the single route's chain of torch kernels performs.
//   Verdicts: with a pointwise type the items of a ROI whose verdict is not 0 write no pointwise row, and no Gradient either
//   when it is PRAD_BINT_NONFINITE (an all-zero box has a native Gradient image of zeros).  Gradient ALONE needs no constants
//   and runs without launch 1: every lane then tests the voxel it centres on, and a float ROI with a value that is not finite
//   gets its verdict from the image launch itself (lanes store the same word); its slice holds the kernel's NaNs until the
//   caller overwrites it from the single route.
//   indices: items, offsets and elements are 64-bit; the split of e into (z, y, x) uses 32-bit divisions when the box holds
//   fewer than 2^32 voxels.  No atomics, no memset.
#pragma once
#include <type_traits>

#include "prad_runtime.h"
#include "wave_reduce.h"

namespace prad {

#define PRAD_BINT_THREADS 256
#define PRAD_BINT_PER_LANE 4
#define PRAD_BINT_CHUNK (PRAD_BINT_THREADS * PRAD_BINT_PER_LANE)
// bit k of `types`: the image types in the order of the rows
#define PRAD_BINT_SQUARE 1
#define PRAD_BINT_SQUAREROOT 2
#define PRAD_BINT_LOGARITHM 4
#define PRAD_BINT_EXPONENTIAL 8
#define PRAD_BINT_GRADIENT 16
#define PRAD_BINT_POINTWISE 15
#define PRAD_BINT_ALL 31
// verdicts
#define PRAD_BINT_ZERO 1
#define PRAD_BINT_NONFINITE 2
// workgroups of one launch: 256 lanes each, and a grid holds fewer than 2^32 lanes
#define PRAD_BINT_MAX_GROUPS 16777215LL

struct BatchIntRoi {
  long long w;      // first work item of the ROI (prefix sum of the box volumes)
  long long n;      // voxels of the box
  long long off;    // first element of the box in the packed image and in every output row
  int nz, ny, nx;
  int pad;
  double inv[3];    // the factor of the differences along z, y, x: 1 / spacing, or 1
};
static_assert(sizeof(BatchIntRoi) == 64, "BatchIntRoi is uploaded as an array of 64-byte records");

// one workgroup of launch 2: the work items [w0, w1) of the batch line; `first` / `last` = the ROIs of items w0 and w1 - 1.  Also
// the row of the table prad_batch_intensity_plan hands out (4 int64).
struct BatchIntItem {
  long long w0, w1, first, last;
};
static_assert(sizeof(BatchIntItem) == 32, "BatchIntItem is 4 int64");

struct BatchIntConsts {
  double c_sq, top, s_log, k_exp;
};

// ---- the planner: host only, pure.  Sizes have been checked (>= 1).  *n_items = the workgroups of launch 2; items (may be NULL)
// ---- receives them.  -> the voxels of the batch
inline long long batch_intensity_plan(const int *sizes, int B, long long *n_items, BatchIntItem *items) {
  long long W = 0;
  for (int b = 0; b < B; b++) W += (long long)sizes[3 * b] * sizes[3 * b + 1] * sizes[3 * b + 2];
  const long long n = (W + PRAD_BINT_CHUNK - 1) / PRAD_BINT_CHUNK;
  *n_items = n;
  if (!items) return W;
  int b = 0;              // the ROI of the item under the cursor; hi = the first item behind it
  long long hi = B > 0 ? (long long)sizes[0] * sizes[1] * sizes[2] : 0;
  auto seek = [&](long long item) {
    while (item >= hi) {
      b++;
      hi += (long long)sizes[3 * b] * sizes[3 * b + 1] * sizes[3 * b + 2];
    }
    return b;
  };
  for (long long c = 0; c < n; c++) {
    BatchIntItem &it = items[c];
    it.w0 = c * PRAD_BINT_CHUNK;
    it.w1 = it.w0 + PRAD_BINT_CHUNK < W ? it.w0 + PRAD_BINT_CHUNK : W;
    it.first = seek(it.w0);
    it.last = seek(it.w1 - 1);      // (the cursor only moves forward: the next chunk starts behind this item)
  }
  return W;
}

#if defined(__HIPCC__)
template <typename TIN>
__global__ void __launch_bounds__(PRAD_BINT_THREADS)
batch_intensity_consts_kernel(const TIN *__restrict__ x, const BatchIntRoi *__restrict__ rois, BatchIntConsts *__restrict__ consts,
                              int *__restrict__ verdict) {
#pragma clang fp contract(off)
  __shared__ double part[PRAD_BINT_THREADS / 64];
  const BatchIntRoi r = rois[blockIdx.x];
  const TIN *__restrict__ box = x + r.off;
  double top = 0.0;
  int bad = 0;
  auto take = [&](TIN v) {
    const double a = fabs((double)v);
    if constexpr (std::is_floating_point<TIN>::value) bad |= !(a <= 1.7976931348623157e308);      // NaN or an infinity
    top = fmax(top, a);
  };
  // four loads in flight per lane (a maximum does not depend on the order it is taken in), then the rest one by one
  long long e = threadIdx.x;
  for (; e + 3 * PRAD_BINT_THREADS < r.n; e += 4 * PRAD_BINT_THREADS) {
    const TIN v0 = box[e], v1 = box[e + PRAD_BINT_THREADS], v2 = box[e + 2 * PRAD_BINT_THREADS], v3 = box[e + 3 * PRAD_BINT_THREADS];
    take(v0);
    take(v1);
    take(v2);
    take(v3);
  }
  for (; e < r.n; e += PRAD_BINT_THREADS) take(box[e]);
  top = wave_max_f64(top);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = top;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < PRAD_BINT_THREADS / 64; k++) top = fmax(top, part[k]);
    BatchIntConsts c;
    c.c_sq = 1.0 / sqrt(top);
    c.top = top;
    c.s_log = top / log(top + 1.0);
    c.k_exp = log(top) / top;
    consts[blockIdx.x] = c;
    verdict[blockIdx.x] = bad ? PRAD_BINT_NONFINITE : (top == 0.0 ? PRAD_BINT_ZERO : 0);
  }
}

template <typename TIN>
__global__ void __launch_bounds__(PRAD_BINT_THREADS)
batch_intensity_kernel(const TIN *__restrict__ x, const BatchIntRoi *__restrict__ rois, const BatchIntItem *__restrict__ items,
                       const BatchIntConsts *__restrict__ consts, int *__restrict__ verdict, int types,
                       double *__restrict__ out64, long long row_stride, float *__restrict__ out_grad) {
#pragma clang fp contract(off)
  const BatchIntItem I = items[blockIdx.x];
  const bool pointwise = (types & PRAD_BINT_POINTWISE) != 0, gradient = (types & PRAD_BINT_GRADIENT) != 0;
#pragma unroll
  for (int k = 0; k < PRAD_BINT_PER_LANE; k++) {
    const long long item = I.w0 + (long long)k * PRAD_BINT_THREADS + threadIdx.x;
    if (item >= I.w1) break;
    int a = (int)I.first, z = (int)I.last;          // the last ROI of [first, last] with w <= item
    while (a < z) {
      const int m = (a + z + 1) >> 1;
      if (rois[m].w <= item) a = m;
      else z = m - 1;
    }
    const BatchIntRoi r = rois[a];
    const long long e = item - r.w;
    const TIN *__restrict__ box = x + r.off;
    const double v = (double)box[e];
    int verd = 0;
    if (pointwise) {
      verd = verdict[a];                            // (launch 1 wrote it)
    } else if constexpr (std::is_floating_point<TIN>::value) {
      if (!(fabs(v) <= 1.7976931348623157e308)) verdict[a] = PRAD_BINT_NONFINITE;      // (Gradient alone: found here)
    }
    if (pointwise && verd == 0) {
      const BatchIntConsts c = consts[a];
      const double sgn = (double)((0.0 < v) - (v < 0.0)), mag = fabs(v);
      double *__restrict__ o = out64 + r.off + e;
      if (types & PRAD_BINT_SQUARE) {
        const double t = c.c_sq * v;
        *o = t * t;
        o += row_stride;
      }
      if (types & PRAD_BINT_SQUAREROOT) {
        *o = sgn * sqrt(mag * c.top);
        o += row_stride;
      }
      if (types & PRAD_BINT_LOGARITHM) {
        *o = (sgn * log(mag + 1.0)) * c.s_log;
        o += row_stride;
      }
      if (types & PRAD_BINT_EXPONENTIAL) *o = exp(c.k_exp * v);
    }
    if (gradient && verd != PRAD_BINT_NONFINITE) {
      long long zz, yy, xx;
      if (r.n <= 0xffffffffLL) {
        const unsigned plane = (unsigned)r.ny * (unsigned)r.nx, e32 = (unsigned)e;
        const unsigned q = e32 / plane, rem = e32 - q * plane, y32 = rem / (unsigned)r.nx;
        zz = q;
        yy = y32;
        xx = rem - y32 * (unsigned)r.nx;
      } else {
        const long long plane = (long long)r.ny * r.nx;
        zz = e / plane;
        const long long rem = e - zz * plane;
        yy = rem / r.nx;
        xx = rem - yy * r.nx;
      }
      const long long sy = r.nx, sz = (long long)r.ny * r.nx;
      double acc = 0.0;
      if (r.nz > 1) {
        const long long up = zz + 1 < r.nz ? sz : 0, dn = zz > 0 ? sz : 0;
        double d = 0.5 * ((double)box[e + up] - (double)box[e - dn]);
        d = d * r.inv[0];
        acc = acc + d * d;
      }
      if (r.ny > 1) {
        const long long up = yy + 1 < r.ny ? sy : 0, dn = yy > 0 ? sy : 0;
        double d = 0.5 * ((double)box[e + up] - (double)box[e - dn]);
        d = d * r.inv[1];
        acc = acc + d * d;
      }
      if (r.nx > 1) {
        const long long up = xx + 1 < r.nx ? 1 : 0, dn = xx > 0 ? 1 : 0;
        double d = 0.5 * ((double)box[e + up] - (double)box[e - dn]);
        d = d * r.inv[2];
        acc = acc + d * d;
      }
      out_grad[r.off + e] = (float)sqrt(acc);
    }
  }
}
#endif  // __HIPCC__

}  // namespace prad
