// kernels_batch_features.h -- the feature formulas of a batch of small ROIs on the flat matrix buffers of the batched matrix
// calls (kernels_batch.h, kernels_batch_glszm.h): two launches for the whole batch instead of six per ROI.
//
//   batch_features_kernel   one workgroup of PRAD_FEAT_THREADS per RECORD of a device table; a record is one matrix the single
//                           calls would evaluate in one workgroup: a GLCM angle, a GLRLM angle, a GLDM, an NGTDM or a GLSZM.
//                           The workgroup reads its record and calls the device function the single-call kernel calls
//                           (kernels_features.h), with the same thread count, on the same matrix values: the same additions
//                           in the same order, the same bits.
//   batch_mcc_kernel        one workgroup of PRAD_MCC_BT per GLCM-angle record (they lead the table): glcm_mcc_block of
//                           kernels_mcc.h, staged, nmax = Ng (Ng <= 64 = PRAD_MCC_NMAX: "too many levels" cannot occur).
// Every output element and every empty flag has exactly one owner workgroup: no atomics, no pre-zeroing.  The marginals of
// the zone-like families live in one global scratch row of Ni + Nj doubles per record (a GLSZM row has up to 54528 columns),
// as in the single call; everything else is LDS: max(5 Ng + 4, 3 Ng + 5, 14 * 4) doubles, under 4 KiB at 64 levels.
#pragma once
#define PRAD_DEVICE_FUNCTIONS_ONLY      // the single-call kernels belong to the translation units that launch them
#include "kernels_features.h"
#include "kernels_mcc.h"
#undef PRAD_DEVICE_FUNCTIONS_ONLY

namespace prad {

enum { BF_GLCM = 0, BF_GLRLM, BF_GLDM, BF_NGTDM, BF_GLSZM, BF_KINDS };
#define PRAD_BF_GLCM_ROW 24      // GF_COUNT sum features + MCC
#define PRAD_BF_MAX_NG 64

struct BatchFeatRec {
  long long mat;        // first element of the ROI's matrix in its family's buffer
  long long scratch;    // first element of the record's scratch row (zone-like kinds)
  long long out;        // first element of the record's output row
  long long sizes;      // GLSZM: first int of the ROI's size list; < 0: the size value of column j is j + 1
  int empty;            // index of the record's empty flag (= its row number)
  int kind, roi, a;     // BF_*, ROI, angle within the ROI's matrix
  int Ni, Nj, Na, pad;  // rows, columns, angles of the matrix
};
static_assert(sizeof(BatchFeatRec) == 64, "one record per 64 bytes");

struct BatchFeatArgs {
  const BatchFeatRec *recs;
  const double *mats[BF_KINDS];
  const int *sizes;
  double *scratch, *out;
  int *empty;
  int symmetric;
  int mcc;             // batch_mcc_kernel follows and owns slot GF_COUNT of every GLCM row; 0: that slot is NaN
};

__host__ __device__ inline size_t batch_features_lds_doubles(int Ng) {
  size_t n = (size_t)5 * Ng + PRAD_FEAT_WAVES;                                  // GLCM marginals + reduction slots
  const size_t ngtdm = (size_t)3 * Ng + PRAD_FEAT_WAVES + 1;                    // level table, slots, the level count
  const size_t zone = (size_t)14 * PRAD_FEAT_WAVES;                             // sh4 + shn
  if (ngtdm > n) n = ngtdm;
  if (zone > n) n = zone;
  return n;
}

__global__ void __launch_bounds__(PRAD_FEAT_THREADS) batch_features_kernel(BatchFeatArgs A) {
  extern __shared__ double bf_lds[];
  const BatchFeatRec r = A.recs[blockIdx.x];
  // (constant indices: a kernel argument array indexed by a variable would go through scratch memory)
  const double *M = (r.kind == BF_GLCM ? A.mats[BF_GLCM] : r.kind == BF_GLRLM ? A.mats[BF_GLRLM] : r.kind == BF_GLDM ? A.mats[BF_GLDM]
                     : r.kind == BF_NGTDM ? A.mats[BF_NGTDM] : A.mats[BF_GLSZM]) + r.mat;
  double *o = A.out + r.out;
  int *e = A.empty + r.empty;
  if (r.kind == BF_GLCM) {
    glcm_features_block(M, r.Ni, r.Na, r.a, A.symmetric, o, e, bf_lds);
    if (!A.mcc && threadIdx.x == 0) o[GF_COUNT] = __builtin_nan("");
  } else if (r.kind == BF_NGTDM) {
    int *ngp = reinterpret_cast<int *>(bf_lds + 3 * r.Ni + PRAD_FEAT_WAVES);
    ngtdm_features_block(M, r.Ni, o, bf_lds, ngp);
    if (threadIdx.x == 0) *e = *ngp == 0;      // (thread 0 wrote the count itself)
  } else {
    // [Ni][Nj][Na] (GLRLM) or [Ni][Nj] (Na = 1): the strides of the single call's contiguous tensor
    const long long sj = r.Na, si = (long long)r.Nj * r.Na;
    const int *sz = (r.kind == BF_GLSZM && r.sizes >= 0) ? A.sizes + r.sizes : nullptr;
    auto jval = [&](int j) -> double { return sz ? (double)sz[j] : (double)(j + 1); };   // (int32 -> double is exact)
    zone_features_block(M, r.Ni, r.Nj, r.a, si, sj, 1LL, jval, A.scratch + r.scratch, o, e, bf_lds, bf_lds + PRAD_FEAT_WAVES);
  }
}

// the first `gridDim.x` records are the GLCM angles; out slot: the last of the angle's PRAD_BF_GLCM_ROW
__global__ void __launch_bounds__(PRAD_MCC_BT) batch_mcc_kernel(BatchFeatArgs A, int *__restrict__ too_many) {
  extern __shared__ double bm_lds[];
  __shared__ double red[PRAD_MCC_BT / 64];
  __shared__ int shn;
  const BatchFeatRec r = A.recs[blockIdx.x];
  glcm_mcc_block(A.mats[BF_GLCM] + r.mat, r.Ni, r.Na, r.a, A.symmetric, r.Ni, 1, A.out + r.out + GF_COUNT, too_many, bm_lds, red,
                 &shn);
}

}  // namespace prad
