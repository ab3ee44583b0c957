// kernels_resegment.h -- resegmentation of ONE volume on the device (prad_resegment_dev): the ROI (labelmap == label) is
// restricted to the voxels whose intensity lies in a range given absolutely, relative to the ROI's maximum or in standard
// deviations about the ROI's mean (radiomics/imageoperations.py:533-640), with the arithmetic numpy applies to the host arrays.
//   reseg_stats_kernel   (relative, sigma)  per workgroup: ROI voxels, their sum, their maximum, a non-finite flag -> partial[g]
//   reseg_ssd_kernel     (sigma)            per workgroup: sum of (x - mean)^2 -> ssd[g]; the mean from the partials
//   reseg_mask_kernel    (every mode)       thresholds from the partials, out = label where kept and 0 elsewhere, counts and
//                                           the box of the kept ROI by integer atomics into the summary
//   reseg_init_kernel    (absolute)         the summary's initial values (the statistics launch sets them in the other modes)
// Work is divided by voxels over the whole grid (a grid-stride loop, 64-bit indices); the grid is a function of the voxel count
// alone and every sum has ONE order -- lane-strided terms, the wave's butterfly, the workgroup's waves in turn, the partials in
// turn (reseg_combine) -- so the thresholds depend on the data alone.  No floating-point atomics.
// The device functions of the comparison and the statistics are shared with kernels_batch_resegment.h.
#pragma once
#include <type_traits>

#include "prad_runtime.h"

namespace prad {

#define PRAD_RESEG_THREADS 256
#define PRAD_RESEG_WAVES (PRAD_RESEG_THREADS / 64)
#define PRAD_RESEG_PER_LANE 16      // voxels a lane takes when the grid is not yet at its cap
#define PRAD_RESEG_MAX_GROUPS 1024  // the cap of the grid = the most partials a workgroup combines

#define PRAD_RESEG_ABSOLUTE 0
#define PRAD_RESEG_RELATIVE 1
#define PRAD_RESEG_SIGMA 2

// the sum of an integer image is an exact 64-bit integer, that of a float image a float64 in a fixed order
template <typename T>
struct ResegSum {
  typedef typename std::conditional<std::is_integral<T>::value, long long, double>::type type;
};

// what a workgroup (single call: of many; batch call: the only one of its ROI) knows about the ROI after the statistics pass
template <typename T>
struct ResegStats {
  long long count;
  typename ResegSum<T>::type sum;
  double top;        // maximum (exact in float64 for every image type); -inf for an empty ROI
  int nonfinite;
  int pad;
};

struct ResegSummary {
  unsigned long long before, after;   // ROI voxels on entry, kept voxels
  int lo[3], hi[3];                   // box of the kept ROI, z y x, inclusive; lo = the sizes, hi = -1 when nothing is kept
  int nonfinite, pad;
  double thr[2];                      // the thresholds (float32 images: the float32 values, widened); thr[1] = +inf for one bound
};
static_assert(sizeof(ResegSummary) == 64, "ResegSummary is read back as 64 bytes");

// the two (sorted) range values and how to use them; passed by value to every kernel
struct ResegRange {
  double t[2];
  int two;       // 1: closed range [t0, t1]; 0: x >= t0 only
  int mode;
};

// host: mode, nrange and the range values of both entry points; *r gets the values sorted as sorted() sorts them
static inline int resegment_range_check(const char *what, int mode, const double *range, int nrange, ResegRange *r) {
  if (mode < PRAD_RESEG_ABSOLUTE || mode > PRAD_RESEG_SIGMA)
    return fail(PRAD_E_ARG, "%s: mode=%d (0 absolute, 1 relative, 2 sigma)", what, mode);
  if (nrange < 1 || nrange > 2) return fail(PRAD_E_ARG, "%s: nrange=%d (1 or 2 thresholds)", what, nrange);
  if (!range) return fail(PRAD_E_ARG, "%s: NULL pointer", what);
  for (int k = 0; k < nrange; k++)
    if (isnan(range[k])) return fail(PRAD_E_ARG, "%s: range[%d] is NaN", what, k);
  r->mode = mode;
  r->two = nrange == 2;
  r->t[0] = range[0];
  r->t[1] = r->two ? range[1] : 0.0;
  if (r->two && r->t[1] < r->t[0]) {
    const double lo = r->t[1];
    r->t[1] = r->t[0];
    r->t[0] = lo;
  }
  return PRAD_OK;
}


template <typename T>
__device__ __forceinline__ bool reseg_finite(T x) {
  if constexpr (std::is_integral<T>::value) return true;
  else return isfinite(x);
}

// numpy compares a float32 array with a Python number in float32 and every other image type in float64; thr holds values
// that are already rounded to the comparison type
template <typename T>
__device__ __forceinline__ bool reseg_keep(T x, const double thr[2], int two) {
  if constexpr (std::is_same<T, float>::value) {
    return x >= (float)thr[0] && (!two || x <= (float)thr[1]);
  } else {
    const double v = (double)x;
    return v >= thr[0] && (!two || v <= thr[1]);
  }
}

// the thresholds of imageoperations.resegmentMask for a ROI of `n` voxels with sum `sum`, maximum `top` and squared deviations
// `ssd` about mean: [f(t) for t in sorted(range)], NOT sorted again (a negative maximum gives a descending pair)
template <typename T>
__device__ __forceinline__ double reseg_mean(const ResegStats<T> &s) {
  return __ddiv_rn((double)s.sum, (double)s.count);      // integer images: one division of the exact sum, as np.mean
}
template <typename T>
__device__ __forceinline__ void reseg_thresholds(const ResegRange &r, const ResegStats<T> &s, double ssd, double thr[2]) {
  const bool f32 = std::is_same<T, float>::value;
  for (int k = 0; k < 2; k++) {
    const double t = r.t[k];
    double v;
    if (r.mode == PRAD_RESEG_ABSOLUTE) {
      v = f32 ? (double)(float)t : t;
    } else if (r.mode == PRAD_RESEG_RELATIVE) {
      // np.float32 * Python float: the number is rounded to float32, then ONE float32 product; otherwise a float64 product
      v = f32 ? (double)__fmul_rn((float)s.top, (float)t) : __dmul_rn(s.top, t);
    } else {
      const double sd = __dsqrt_rn(__ddiv_rn(ssd, (double)s.count));      // population sigma, np.std's ddof = 0
      v = __dadd_rn(reseg_mean(s), __dmul_rn(sd, t));                      // (no contraction: numpy rounds the product)
    }
    thr[k] = v;
  }
  if (!r.two) thr[1] = __builtin_inf();
}

// ---- the workgroup's reductions: every thread gets the result, in one fixed order -----------------------------------------
template <typename V>
__device__ __forceinline__ V reseg_wave_sum(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// scratch: PRAD_RESEG_WAVES values of 8 bytes in LDS; two barriers, so the scratch is free again on return
template <typename V>
__device__ __forceinline__ V reseg_block_sum(V v, void *scratch) {
  static_assert(sizeof(V) == 8, "8-byte terms");
  V *s = (V *)scratch;
  v = reseg_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  V total = s[0];
#pragma unroll
  for (int w = 1; w < PRAD_RESEG_WAVES; w++) total += s[w];
  __syncthreads();
  return total;
}
__device__ __forceinline__ double reseg_block_max(double v, void *scratch) {
  double *s = (double *)scratch;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double top = s[0];
#pragma unroll
  for (int w = 1; w < PRAD_RESEG_WAVES; w++) top = fmax(top, s[w]);
  __syncthreads();
  return top;
}

// one lane's terms -> the workgroup's statistics (all threads)
template <typename T>
__device__ __forceinline__ ResegStats<T> reseg_block_stats(long long count, typename ResegSum<T>::type sum, double top, int bad,
                                                           void *scratch) {
  ResegStats<T> s;
  s.count = reseg_block_sum<long long>(count, scratch);
  s.sum = reseg_block_sum<typename ResegSum<T>::type>(sum, scratch);
  s.top = reseg_block_max(top, scratch);
  s.nonfinite = reseg_block_sum<long long>((long long)bad, scratch) != 0;
  s.pad = 0;
  return s;
}

// the partials of `groups` workgroups combined in the order of their numbers: lane l of every wave takes partials l, l + 64,
// ... in turn, then the butterfly.  Every wave of every workgroup computes the same value.
template <typename T>
__device__ __forceinline__ ResegStats<T> reseg_combine(const ResegStats<T> *__restrict__ partial, int groups) {
  long long count = 0;
  typename ResegSum<T>::type sum = 0;
  double top = -__builtin_inf();
  int bad = 0;
  for (int g = threadIdx.x & 63; g < groups; g += 64) {
    const ResegStats<T> p = partial[g];
    count += p.count;
    sum += p.sum;
    top = fmax(top, p.top);
    bad |= p.nonfinite;
  }
  ResegStats<T> s;
  s.count = reseg_wave_sum(count);
  s.sum = reseg_wave_sum(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o));
  s.top = top;
  s.nonfinite = reseg_wave_sum(bad) != 0;
  s.pad = 0;
  return s;
}
__device__ __forceinline__ double reseg_combine_ssd(const double *__restrict__ ssd, int groups) {
  double v = 0.0;
  for (int g = threadIdx.x & 63; g < groups; g += 64) v += ssd[g];
  return reseg_wave_sum(v);
}

__device__ __forceinline__ void reseg_summary_init(ResegSummary *sum, int nz, int ny, int nx) {
  sum->before = sum->after = 0ull;
  sum->lo[0] = nz;
  sum->lo[1] = ny;
  sum->lo[2] = nx;
  sum->hi[0] = sum->hi[1] = sum->hi[2] = -1;
  sum->nonfinite = sum->pad = 0;
  sum->thr[0] = sum->thr[1] = 0.0;
}

// ---- the kernels of the single call -------------------------------------------------------------------------------------------
struct ResegGeo {
  long long n;      // voxels (make_geo: below 2^31)
  int nz, ny, nx;   // leading extents 1 for Nd < 3
  int groups;       // workgroups of every launch of the call
};

static __global__ void reseg_init_kernel(ResegSummary *sum, ResegGeo g) { reseg_summary_init(sum, g.nz, g.ny, g.nx); }

template <typename T, typename L>
__global__ void __launch_bounds__(PRAD_RESEG_THREADS)
reseg_stats_kernel(const T *__restrict__ image, const L *__restrict__ lab, ResegGeo g, int label, ResegStats<T> *__restrict__ partial,
                   ResegSummary *sum) {
  __shared__ double scratch[PRAD_RESEG_WAVES];
  long long count = 0;
  typename ResegSum<T>::type acc = 0;
  double top = -__builtin_inf();
  int bad = 0;
  const long long step = (long long)gridDim.x * PRAD_RESEG_THREADS;
  for (long long i = (long long)blockIdx.x * PRAD_RESEG_THREADS + threadIdx.x; i < g.n; i += step) {
    if ((int)lab[i] != label) continue;
    const T x = image[i];
    count++;
    acc += (typename ResegSum<T>::type)x;
    top = fmax(top, (double)x);      // (a NaN is skipped here and flagged below)
    bad |= !reseg_finite(x);
  }
  const ResegStats<T> s = reseg_block_stats<T>(count, acc, top, bad, scratch);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    if (blockIdx.x == 0) reseg_summary_init(sum, g.nz, g.ny, g.nx);      // (the mask launch, later on the stream, adds to it)
  }
}

template <typename T, typename L>
__global__ void __launch_bounds__(PRAD_RESEG_THREADS)
reseg_ssd_kernel(const T *__restrict__ image, const L *__restrict__ lab, ResegGeo g, int label,
                 const ResegStats<T> *__restrict__ partial, double *__restrict__ ssd) {
  __shared__ double scratch[PRAD_RESEG_WAVES];
  const ResegStats<T> s = reseg_combine<T>(partial, g.groups);
  const double mean = reseg_mean(s);
  double acc = 0.0;
  const long long step = (long long)gridDim.x * PRAD_RESEG_THREADS;
  for (long long i = (long long)blockIdx.x * PRAD_RESEG_THREADS + threadIdx.x; i < g.n; i += step) {
    if ((int)lab[i] != label) continue;
    const double d = __dsub_rn((double)image[i], mean);
    acc = __dadd_rn(acc, __dmul_rn(d, d));      // np.std squares, then sums
  }
  const double total = reseg_block_sum<double>(acc, scratch);
  if (threadIdx.x == 0) ssd[blockIdx.x] = total;
}

template <typename T, typename L>
__global__ void __launch_bounds__(PRAD_RESEG_THREADS)
reseg_mask_kernel(const T *__restrict__ image, const L *__restrict__ lab, ResegGeo g, int label, ResegRange r,
                  const ResegStats<T> *__restrict__ partial, const double *__restrict__ ssd, L *__restrict__ out, ResegSummary *sum) {
  __shared__ double scratch[PRAD_RESEG_WAVES];
  ResegStats<T> s;
  s.count = 0;
  s.sum = 0;
  s.top = 0.0;
  s.nonfinite = s.pad = 0;
  double dev2 = 0.0;
  if (r.mode != PRAD_RESEG_ABSOLUTE) s = reseg_combine<T>(partial, g.groups);
  if (r.mode == PRAD_RESEG_SIGMA) dev2 = reseg_combine_ssd(ssd, g.groups);
  double thr[2];
  reseg_thresholds<T>(r, s, dev2, thr);

  long long before = 0, after = 0;
  int lo_z = g.nz, lo_y = g.ny, lo_x = g.nx, hi_z = -1, hi_y = -1, hi_x = -1, bad = 0;
  const unsigned plane = (unsigned)g.ny * (unsigned)g.nx;      // (n < 2^31: 32-bit divisions)
  const long long step = (long long)gridDim.x * PRAD_RESEG_THREADS;
  for (long long i = (long long)blockIdx.x * PRAD_RESEG_THREADS + threadIdx.x; i < g.n; i += step) {
    L o = (L)0;
    if ((int)lab[i] == label) {
      const T x = image[i];
      before++;
      bad |= !reseg_finite(x);
      if (reseg_keep<T>(x, thr, r.two)) {
        o = (L)label;
        after++;
        const unsigned e = (unsigned)i, z = e / plane, rem = e - z * plane, y = rem / (unsigned)g.nx, x0 = rem - y * (unsigned)g.nx;
        lo_z = min(lo_z, (int)z);
        lo_y = min(lo_y, (int)y);
        lo_x = min(lo_x, (int)x0);
        hi_z = max(hi_z, (int)z);
        hi_y = max(hi_y, (int)y);
        hi_x = max(hi_x, (int)x0);
      }
    }
    out[i] = o;
  }
  // the workgroup's counts, then one lane per wave with a kept voxel updates the box: integer atomics, exact in any order
  before = reseg_block_sum<long long>(before, scratch);
  after = reseg_block_sum<long long>(after, scratch);
  const long long flagged = reseg_block_sum<long long>((long long)bad, scratch);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo_z = min(lo_z, __shfl_xor(lo_z, o));
    lo_y = min(lo_y, __shfl_xor(lo_y, o));
    lo_x = min(lo_x, __shfl_xor(lo_x, o));
    hi_z = max(hi_z, __shfl_xor(hi_z, o));
    hi_y = max(hi_y, __shfl_xor(hi_y, o));
    hi_x = max(hi_x, __shfl_xor(hi_x, o));
  }
  if ((threadIdx.x & 63) == 0 && hi_z >= 0) {
    atomicMin(&sum->lo[0], lo_z);
    atomicMin(&sum->lo[1], lo_y);
    atomicMin(&sum->lo[2], lo_x);
    atomicMax(&sum->hi[0], hi_z);
    atomicMax(&sum->hi[1], hi_y);
    atomicMax(&sum->hi[2], hi_x);
  }
  if (threadIdx.x == 0) {
    if (before) atomicAdd(&sum->before, (unsigned long long)before);
    if (after) atomicAdd(&sum->after, (unsigned long long)after);
    if (flagged || s.nonfinite) atomicOr(&sum->nonfinite, 1);
    if (blockIdx.x == 0) {
      sum->thr[0] = thr[0];
      sum->thr[1] = thr[1];
    }
  }
}

}  // namespace prad
