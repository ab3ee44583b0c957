// kernels_batch_log.h -- the Laplacian-of-Gaussian images of MANY small boxes in a few launches (gfx950): ITK's
// LaplacianRecursiveGaussianImageFilter with NormalizeAcrossScale on every box alone, as log_multi_dev (prad_filters.hip) runs
// it on one box -- per ROI and sigma the bits of that route -- on the batch layout of kernels_batch_firstorder.h.
//
// batch_log_kernel<TIN>.  One workgroup per ITEM = one (ROI, sigma) pair; ROI b is the box [Nz][Ny][Nx] at element `off` of the
// packed image (TIN: float32 / float64 / int32 / int16), its image for sigma row s goes to out + s * row_stride + off in the
// box's own shape: float64 for a float64 input, float32 otherwise.
//   order     ITK's (log_multi_dev): terms for dim = x, y, z; a term is the order-2 pass along dim, which reads the INPUT in its
//             own type widened to float64 (exact for all four types), then the order-0 passes along the other two axes in x, y, z
//             order; the image between the passes is float32; after a term  acc = (float)((double)acc + (double)term /
//             spacing[dim]^2), from 0 (log_combine_kernel); the last acc is cast to the output type.
//   image     the working image is a float32 copy of the box in LDS, [Nz][Ny][PX] with the odd row pitch PX = Nx | 1: the lanes
//             of an x pass (one line each, PX floats apart) fall on 32 different banks; in the y and z passes neighbouring lanes
//             are neighbouring x.  The derivative pass reads the box from global memory (three times per item: the workgroup read
//             it moments before) and writes LDS; the smoothing passes run in place, a lane owns its line.  The accumulator lives
//             in the item's own slice of `out` (a float32 value passes through a float64 slot exactly); each voxel of it is
//             read and written by the same lane in all three terms.
//   line      the arithmetic of rgauss_line_kernel (kernels_filters.h) sample by sample -- the four-sample boundary
//             initialisation at both ends, every sum in its association, contraction off -- in the schedule of
//             rgauss_pass_kernel: sweep 1 runs the anti-causal recursion from the end of the line and keeps its four values at
//             the block boundaries 16, 32 and 48 in registers (a line has at most 64 samples); sweep 2 walks forward in blocks
//             of 16 (the last one 4 .. 19), causal recursion into registers, the anti-causal one of the block recomputed
//             downward from the kept state (the same operations on the same operands), sum, round to float32, store.  A block
//             is stored after its last read and the three samples the next block's causal numerator needs travel in
//             registers, so a pass may overwrite its own input.
//   domain    a ROI is native (blog_roi_native) when every extent lies in [4, 64] and the padded image, 4 Nz Ny (Nx | 1)
//             bytes -- all the LDS the kernel uses --, fits the 160 KiB of a compute unit: 32^3 (135 168 B) is, 36^3 (191 808 B)
//             is not.  Whether the reference yields an image at all for a (ROI, sigma) pair is the planner's second question
//             (batch_log_plan below).
//   classes   dynamic LDS is one number per launch: the native ROIs are sorted into three classes by footprint (<= 16 KiB,
//             <= 64 KiB, above), each class is one launch with the largest footprint among its ROIs and its own workgroup size
//             (256, 512, 768 lanes: 16^3 has 256 lines per pass, 32^3 has 1024), so a thousand 8^3 boxes next to one 32^3 box
//             keep their residency.  768 lanes leave the kernel its 150-odd registers (three waves per SIMD, no scratch); with
//             1024 the budget is 128 and the compiler spills ~120 B per lane: 1.23 ms against 1.01 ms for 256 boxes of 32^3.
//   traffic   no atomics, no memset; a workgroup writes only its own ROI's slice of its own sigma's row.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): see DESIGN.md, "LoG images of a batch
// of boxes".
#pragma once
#include <cmath>
#include <type_traits>

#include "prad_rgauss.h"
#include "prad_runtime.h"

namespace prad {

#define PRAD_BLOG_MIN_EXTENT 4
#define PRAD_BLOG_MAX_EXTENT 64
#define PRAD_BLOG_MAX_LDS (160 * 1024)
// lanes of the workgroups of the three LDS classes
#define PRAD_BLOG_THREADS_0 256
#define PRAD_BLOG_THREADS_1 512
#ifndef PRAD_BLOG_THREADS_2
#define PRAD_BLOG_THREADS_2 768      // (measured against 512 and 1024: profiles/batch_log_measurements.md)
#endif
#define PRAD_BLOG_MAXSIG 8           // sigmas per call (PRAD_LOG_MAXSIG of the single route)
#define PRAD_BLOG_CLASSES 3
// verdict of a (ROI, sigma) pair: 0 computed by the launch, 8 outside the kernel's domain -- the single route serves the pair --,
// PRAD_BLOG_NO_IMAGE the reference yields no image for it (getLoGImage: an extent below 4, "Image too small", or below
// ceil(sigma / spacing) + 1)
#define PRAD_BLOG_SINGLE 8
#define PRAD_BLOG_NO_IMAGE 16

struct BatchLogRoi {
  long long off;      // first element of the box in the packed image and in every row of the output
  int nz, ny, nx;
  int pad;
  double sp2[3];      // spacing^2 of the array axes z, y, x
};
static_assert(sizeof(BatchLogRoi) == 48, "BatchLogRoi is uploaded as an array of 48-byte records");

struct BatchLogItem {
  int roi, row;       // the ROI and the row of `out` (the sigma)
  int c2[3], c0[3];   // index of the order-2 / order-0 coefficients of this sigma along the array axes z, y, x
};
static_assert(sizeof(BatchLogItem) == 32, "BatchLogItem is 8 ints");

// ---- the planner: host only, pure -------------------------------------------------------------------------------------------
// bytes of LDS of a box: the float32 image with the odd row pitch
inline long long blog_footprint(const int *size) { return 4LL * size[0] * size[1] * (size[2] | 1); }
inline bool blog_roi_native(const int *size) {
  for (int d = 0; d < 3; d++)
    if (size[d] < PRAD_BLOG_MIN_EXTENT || size[d] > PRAD_BLOG_MAX_EXTENT) return false;
  return blog_footprint(size) <= PRAD_BLOG_MAX_LDS;
}
// the class of a native box by its footprint
inline int blog_lds_class(const int *size) {
  const long long f = blog_footprint(size);
  return f <= 16 * 1024 ? 0 : f <= 64 * 1024 ? 1 : 2;
}
// the reference's admission of a pair (imageoperations.py getLoGImage): every extent >= 4 and >= ceil(sigma / spacing) + 1
inline bool blog_reference_has_image(const int *size, const double *spacing, double sigma) {
  for (int d = 0; d < 3; d++)
    if (size[d] < 4 || (double)size[d] < std::ceil(sigma / spacing[d]) + 1.0) return false;
  return true;
}
// verdict int [S][B]; lds_class int [B]: the class of a native ROI, -1 for any other; *n_items = the zeros of verdict.  A box
// that cannot be native because it is too LARGE (an extent above 64, or the LDS) is 8 for every sigma: the single route, which
// asks the reference's question itself, decides about it.  Every other box gets the reference's answer per sigma: no image, or
// 0.  Sizes, sigmas and spacings have been checked (> 0).
inline void batch_log_plan(const int *sizes, int B, const double *spacing, const double *sigmas, int S, int *verdict,
                           int *lds_class, long long *n_items) {
  long long n = 0;
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    const bool native = blog_roi_native(sz);
    const bool large = !native && sz[0] >= PRAD_BLOG_MIN_EXTENT && sz[1] >= PRAD_BLOG_MIN_EXTENT && sz[2] >= PRAD_BLOG_MIN_EXTENT;
    const bool beyond = sz[0] > PRAD_BLOG_MAX_EXTENT || sz[1] > PRAD_BLOG_MAX_EXTENT || sz[2] > PRAD_BLOG_MAX_EXTENT;
    if (lds_class) lds_class[b] = native ? blog_lds_class(sz) : -1;
    for (int s = 0; s < S; s++) {
      int v;
      if (large || beyond) v = PRAD_BLOG_SINGLE;
      else v = blog_reference_has_image(sz, spacing + 3 * b, sigmas[s]) ? 0 : PRAD_BLOG_NO_IMAGE;
      if (verdict) verdict[(long long)s * B + b] = v;
      n += v == 0;
    }
  }
  if (n_items) *n_items = n;
}

#if defined(__HIPCC__)
// One line of ITK's RecursiveSeparableImageFilter::FilterDataArray: d(i), 0 <= i < ln, reads sample i as float64; sample i of
// the result goes to w[i * wst] as float32.  4 <= ln <= 64.  d may read w itself (see "line" above).
template <typename D>
__host__ __device__ __forceinline__ void blog_line(const D &d, const int ln, float *w, const int wst, const RGaussCoef &c) {
#pragma clang fp contract(off)  // ITK's line arithmetic is plain multiply / add; keep the same roundings
  constexpr int RB = 16, RM = RB + 4;
  const int nb = (ln - 4) / RB + 1;        // blocks [k RB, (k + 1) RB) for k < nb - 1; the last takes the rest, 4 .. RB + 3
  // the state of boundary k = 1 .. 3: anticausal[k RB .. k RB + 3]
  double sa0 = 0, sa1 = 0, sa2 = 0, sa3 = 0, sb0 = 0, sb1 = 0, sb2 = 0, sb3 = 0, sc0 = 0, sc1 = 0, sc2 = 0, sc3 = 0;
  // ---- sweep 1: anti-causal, from the end, states only ----
  {
    const double v2 = d(ln - 1), y1 = d(ln - 2), y2 = d(ln - 3);
    double a1 = v2 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;     // index ln-1
    double a2 = v2 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;     // index ln-2
    double a3 = y1 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;     // index ln-3
    double a4 = y2 * c.M1 + y1 * c.M2 + v2 * c.M3 + v2 * c.M4;     // index ln-4
    a1 -= v2 * c.BM1 + v2 * c.BM2 + v2 * c.BM3 + v2 * c.BM4;
    a2 -= a1 * c.D1 + v2 * c.BM2 + v2 * c.BM3 + v2 * c.BM4;
    a3 -= a2 * c.D1 + a1 * c.D2 + v2 * c.BM3 + v2 * c.BM4;
    a4 -= a3 * c.D1 + a2 * c.D2 + a1 * c.D3 + v2 * c.BM4;
    double dp0 = d(ln - 4), dp1 = y2, dp2 = y1, dp3 = v2;            // data[i .. i+3] at i = ln-4
    double q0 = a4, q1 = a3, q2 = a2, q3 = a1;                       // anticausal[i .. i+3]
    // q0 = anticausal[i]: kept where i is a block boundary
#define PRAD_BLOG_KEEP(i)                                          \
  do {                                                             \
    const bool k1 = (i) == RB, k2 = (i) == 2 * RB, k3 = (i) == 3 * RB; \
    sa0 = k1 ? q0 : sa0; sa1 = k1 ? q1 : sa1; sa2 = k1 ? q2 : sa2; sa3 = k1 ? q3 : sa3; \
    sb0 = k2 ? q0 : sb0; sb1 = k2 ? q1 : sb1; sb2 = k2 ? q2 : sb2; sb3 = k2 ? q3 : sb3; \
    sc0 = k3 ? q0 : sc0; sc1 = k3 ? q1 : sc1; sc2 = k3 ? q2 : sc2; sc3 = k3 ? q3 : sc3; \
  } while (0)
    PRAD_BLOG_KEEP(ln - 4);
    for (int i = ln - 4; i > RB; i--) {                              // (block 0's anti-causal part is recomputed in sweep 2)
      double v = dp0 * c.M1 + dp1 * c.M2 + dp2 * c.M3 + dp3 * c.M4;
      v -= q0 * c.D1 + q1 * c.D2 + q2 * c.D3 + q3 * c.D4;
      dp3 = dp2; dp2 = dp1; dp1 = dp0; dp0 = d(i - 1);
      q3 = q2; q2 = q1; q1 = q0; q0 = v;
      PRAD_BLOG_KEEP(i - 1);
    }
#undef PRAD_BLOG_KEEP
  }
  // ---- sweep 2: forward, block by block ----
  double p1 = 0, p2 = 0, p3 = 0, p4 = 0;        // causal[b-1 .. b-4]
  double dm1 = 0, dm2 = 0, dm3 = 0;             // data[b-1 .. b-3]
#pragma unroll 1
  for (int kb = 0; kb < nb; kb++) {
    const int b = kb * RB;
    const bool lastblk = kb == nb - 1;
    const int len = lastblk ? ln - b : RB;      // RB, or 4 .. RB + 3 for the last block
    double cv[RM];
#pragma unroll
    for (int j = 0; j < RM; j++) cv[j] = 0.0;
    int j0 = 0;
    if (kb == 0) {                              // causal start (FilterDataArray)
      const double v1 = d(0);
      const double x1 = d(1), x2 = d(2), x3 = d(3);
      double s0 = v1 * c.N0 + v1 * c.N1 + v1 * c.N2 + v1 * c.N3;
      double s1 = x1 * c.N0 + v1 * c.N1 + v1 * c.N2 + v1 * c.N3;
      double s2 = x2 * c.N0 + x1 * c.N1 + v1 * c.N2 + v1 * c.N3;
      double s3 = x3 * c.N0 + x2 * c.N1 + x1 * c.N2 + v1 * c.N3;
      s0 -= v1 * c.BN1 + v1 * c.BN2 + v1 * c.BN3 + v1 * c.BN4;
      s1 -= s0 * c.D1 + v1 * c.BN2 + v1 * c.BN3 + v1 * c.BN4;
      s2 -= s1 * c.D1 + s0 * c.D2 + v1 * c.BN3 + v1 * c.BN4;
      s3 -= s2 * c.D1 + s1 * c.D2 + s0 * c.D3 + v1 * c.BN4;
      cv[0] = s0; cv[1] = s1; cv[2] = s2; cv[3] = s3;
      dm1 = x3; dm2 = x2; dm3 = x1;
      p1 = s3; p2 = s2; p3 = s1; p4 = s0;
      j0 = 4;
    }
#pragma unroll
    for (int j = 0; j < RM; j++) {
      if (j >= j0 && j < len) {
        const double di = d(b + j);
        double v = di * c.N0 + dm1 * c.N1 + dm2 * c.N2 + dm3 * c.N3;
        v -= p1 * c.D1 + p2 * c.D2 + p3 * c.D3 + p4 * c.D4;
        cv[j] = v;
        dm3 = dm2; dm2 = dm1; dm1 = di;
        p4 = p3; p3 = p2; p2 = p1; p1 = v;
      }
    }
    // anti-causal recursion of the block, downward, from the kept state (or from the end of the line)
    double q0, q1, q2, q3, e0, e1, e2, e3;      // anticausal[i .. i+3], data[i .. i+3] at i = b + len
    int jtop = len - 1;                         // block-local index of the first sample still to produce
    if (lastblk) {
      const double v2 = d(ln - 1), y1 = d(ln - 2), y2 = d(ln - 3), y3 = d(ln - 4);
      double a1 = v2 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;
      double a2 = v2 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;
      double a3 = y1 * c.M1 + v2 * c.M2 + v2 * c.M3 + v2 * c.M4;
      double a4 = y2 * c.M1 + y1 * c.M2 + v2 * c.M3 + v2 * c.M4;
      a1 -= v2 * c.BM1 + v2 * c.BM2 + v2 * c.BM3 + v2 * c.BM4;
      a2 -= a1 * c.D1 + v2 * c.BM2 + v2 * c.BM3 + v2 * c.BM4;
      a3 -= a2 * c.D1 + a1 * c.D2 + v2 * c.BM3 + v2 * c.BM4;
      a4 -= a3 * c.D1 + a2 * c.D2 + a1 * c.D3 + v2 * c.BM4;
      // the four end samples are final here
#pragma unroll
      for (int j = 0; j < RM; j++) {
        if (j == len - 1) cv[j] += a1;
        if (j == len - 2) cv[j] += a2;
        if (j == len - 3) cv[j] += a3;
        if (j == len - 4) cv[j] += a4;
      }
      q0 = a4; q1 = a3; q2 = a2; q3 = a1;
      e0 = y3; e1 = y2; e2 = y1; e3 = v2;
      jtop = len - 5;
    } else {
      q0 = kb == 0 ? sa0 : kb == 1 ? sb0 : sc0;
      q1 = kb == 0 ? sa1 : kb == 1 ? sb1 : sc1;
      q2 = kb == 0 ? sa2 : kb == 1 ? sb2 : sc2;
      q3 = kb == 0 ? sa3 : kb == 1 ? sb3 : sc3;
      e0 = d(b + RB); e1 = d(b + RB + 1); e2 = d(b + RB + 2); e3 = d(b + RB + 3);
    }
#pragma unroll
    for (int jj = RM - 1; jj >= 0; jj--) {
      if (jj <= jtop) {
        double v = e0 * c.M1 + e1 * c.M2 + e2 * c.M3 + e3 * c.M4;
        v -= q0 * c.D1 + q1 * c.D2 + q2 * c.D3 + q3 * c.D4;
        cv[jj] += v;
        e3 = e2; e2 = e1; e1 = e0; e0 = d(b + jj);
        q3 = q2; q2 = q1; q1 = q0; q0 = v;
      }
    }
#pragma unroll
    for (int j = 0; j < RM; j++)
      if (j < len) w[(b + j) * wst] = (float)cv[j];
  }
}

// The lines of one pass along array axis ax (0 z, 1 y, 2 x) that lane tid of nthreads takes.  box: the ROI's input; W: the
// working image [nz][ny][px].  FIRST: the pass reads the input (the derivative pass of a term), else W itself.  Line l starts at
// element gb of the box and wb of W; its samples are gs / ws elements apart.  (Host-callable: the CPU checks run these very
// functions lane by lane.)
template <bool FIRST, typename TIN>
__host__ __device__ __forceinline__ void blog_pass(const TIN *box, float *W, int nz, int ny, int nx, int ax, const RGaussCoef &c,
                                                   int tid, int nthreads) {
  const int px = nx | 1;
  const int ln = ax == 0 ? nz : ax == 1 ? ny : nx;
  const int lines = ax == 0 ? ny * nx : ax == 1 ? nz * nx : nz * ny;
  const int gs = ax == 0 ? ny * nx : ax == 1 ? nx : 1;
  const int ws = ax == 0 ? ny * px : ax == 1 ? px : 1;
  for (int l = tid; l < lines; l += nthreads) {
    int gb, wb;
    if (ax == 2) {
      gb = l * nx;
      wb = l * px;
    } else {
      const int hi = l / nx, lo = l - hi * nx;
      gb = ax == 1 ? hi * ny * nx + lo : l;
      wb = ax == 1 ? hi * ny * px + lo : hi * px + lo;
    }
    float *w = W + wb;
    if (FIRST) {
      const TIN *g = box + gb;
      blog_line([&](int i) { return (double)g[i * gs]; }, ln, w, ws, c);
    } else {
      blog_line([&](int i) { return (double)w[i * ws]; }, ln, w, ws, c);
    }
  }
}

// acc = (float)((double)acc + (double)term / spacing^2) for the voxels of lane tid, acc in the item's slice o of the output
// (FROM_ZERO: the first term; acc starts from 0 and o is not read)
template <typename TOUT>
__host__ __device__ __forceinline__ void blog_accumulate(const float *W, TOUT *o, int nvox, int nx, double sp2, bool from_zero,
                                                         int tid, int nthreads) {
#pragma clang fp contract(off)
  const int px = nx | 1;
  for (int e = tid; e < nvox; e += nthreads) {
    const int zy = e / nx, x = e - zy * nx;
    const float term = W[zy * px + x];
    float acc = from_zero ? 0.0f : (float)o[e];
    acc = (float)((double)acc + (double)term / sp2);
    o[e] = (TOUT)acc;
  }
}

template <typename TIN>
struct BlogOut {
  using type = typename std::conditional<std::is_same<TIN, double>::value, double, float>::type;
};

// MAXT: the lanes of the workgroups of the launch's class (the register budget follows from it)
template <typename TIN, int MAXT>
__global__ void __launch_bounds__(MAXT)
batch_log_kernel(const TIN *__restrict__ in, const BatchLogRoi *__restrict__ rois, const BatchLogItem *__restrict__ items,
                 const RGaussCoef *__restrict__ coefs, void *__restrict__ out, long long row_stride) {
  using TOUT = typename BlogOut<TIN>::type;
  extern __shared__ float blog_lds[];
  float *W = blog_lds;
  const BatchLogItem I = items[blockIdx.x];
  const BatchLogRoi R = rois[I.roi];
  const int nz = R.nz, ny = R.ny, nx = R.nx;
  const int tid = threadIdx.x, nthreads = blockDim.x;
  const TIN *box = in + R.off;
  TOUT *o = (TOUT *)out + (long long)I.row * row_stride + R.off;
#pragma unroll 1
  for (int t = 0; t < 3; t++) {
    const int dim = 2 - t;                      // ITK's x, y, z = array axes 2, 1, 0
    blog_pass<true>(box, W, nz, ny, nx, dim, coefs[dim == 0 ? I.c2[0] : dim == 1 ? I.c2[1] : I.c2[2]], tid, nthreads);
    __syncthreads();
#pragma unroll 1
    for (int other = 2; other >= 0; other--) {
      if (other == dim) continue;
      blog_pass<false>(box, W, nz, ny, nx, other, coefs[other == 0 ? I.c0[0] : other == 1 ? I.c0[1] : I.c0[2]], tid, nthreads);
      __syncthreads();
    }
    blog_accumulate(W, o, nz * ny * nx, nx, dim == 0 ? R.sp2[0] : dim == 1 ? R.sp2[1] : R.sp2[2], t == 0, tid, nthreads);
    __syncthreads();
  }
}
#endif  // __HIPCC__

}  // namespace prad
