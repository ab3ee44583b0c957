// kernels_batch_merge.h -- the weighted angle merge of a batch of small ROIs (weightingNorm): ONE launch turns the per-angle
// GLCM [Ng][Ng][Na] and GLRLM [Ng][Nr][Na1] of every ROI (the flat buffers of kernels_batch.h) into one matrix per ROI,
//     glcm_w[i][j]  = sum_a w_a * (P[i][j][a] + (symmetric ? P[j][i][a] : 0))        float64 [Ng][Ng][1]
//     glrlm_w[i][r] = sum_a w_a * R[i][r][a]                                         float64 [Ng][Nr][1]
// laid out ROI after ROI in flat buffers, so that the feature launch (kernels_batch_features.h) runs on them with one angle
// per ROI and symmetric = 0.
//
// Work is divided by OUTPUT CELLS, not by ROI: a record of the device table names up to PRAD_BM_CELLS consecutive cells of
// one matrix of one ROI, one workgroup of PRAD_BM_THREADS takes a record, a thread owns a cell and walks its angles.  A batch
// of 64-level ROIs so gives 4 workgroups per GLCM however few ROIs it holds, and a 1 x 1 x 1 box costs one record per family.
// Every output element has exactly one writer and is written -- a ROI without angles (Na = 0) or with a status other than
// PRAD_OK gets zeros -- so nothing is zeroed beforehand and there are no atomics.
//
// Arithmetic.  The sum runs over a ascending from 0.0; a term is a ROUNDED product followed by a ROUNDED add, the transpose
// is added first (counts: exact).  Contraction is switched off for the function that forms the sum (#pragma clang fp
// contract(off) over plain * and +: HIP's __dmul_rn / __dadd_rn are ordinary inline operators, which the device compiler's
// default -ffp-contract=fast fuses into v_fma_f64 like any others).  The result is a function of the inputs alone -- not of
// the launch geometry -- and equals a host loop `acc = acc + P[..., a] * w[a]` bit for bit.
//
// Memory.  The angles of a cell are adjacent doubles, so a thread reads Na consecutive doubles and the 64 lanes of a wave
// cover one contiguous piece of 64 * Na doubles: every byte of every line fetched is used by the wave that fetched it.  The
// transposed operand of a symmetric GLCM is strided by Ng * Na doubles between lanes; it is the matrix the same launch reads
// row-wise, at most 64 * 64 * 127 doubles, and comes from L2.  The weights are uniform across the workgroup (scalar loads).
#pragma once
#include "prad_runtime.h"

namespace prad {

#define PRAD_BM_THREADS 256
#define PRAD_BM_CELLS 1024      // cells of one record: four per thread

enum { BM_GLCM = 0, BM_GLRLM = 1 };

struct BatchMergeRec {
  long long in;         // first double of the ROI's per-angle matrix in its family's buffer
  long long out;        // first double of the ROI's merged matrix
  long long w;          // first weight of the ROI's angles of this family in the weight table
  int cell0, ncell;     // the record's cells: cell0 .. cell0 + ncell - 1 of the matrix (row-major [Ni][Nj])
  int nj;               // columns (GLCM: Ng, the transpose of cell i * nj + j is j * nj + i)
  int na;               // angles of the per-angle matrix
  int kind, roi;        // BM_*, ROI (index into status)
};
static_assert(sizeof(BatchMergeRec) == 48, "records are packed");

struct BatchMergeArgs {
  const BatchMergeRec *recs;
  const double *glcm, *glrlm;      // per-angle matrices
  const double *weights;
  const int *status;               // int [B] of the matrix call, or NULL: every ROI counts
  double *glcm_w, *glrlm_w;
  int symmetric;
};

// sum_a w[a] * (p[a] (+ q[a])) over a ascending: a rounded product, then a rounded add, never an FMA
__device__ __forceinline__ double bm_weighted_sum(const double *p, const double *q, const double *w, int na, bool both) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int a = 0; a < na; a++) {
    double t = p[a];
    if (both) t = t + q[a];
    const double term = t * w[a];
    acc = acc + term;
  }
  return acc;
}

__global__ void __launch_bounds__(PRAD_BM_THREADS) batch_merge_kernel(BatchMergeArgs A) {
  const BatchMergeRec r = A.recs[blockIdx.x];
  const bool live = r.na > 0 && (!A.status || A.status[r.roi] == PRAD_OK);
  const double *M = (r.kind == BM_GLCM ? A.glcm : A.glrlm) + r.in;
  double *o = (r.kind == BM_GLCM ? A.glcm_w : A.glrlm_w) + r.out;
  const double *w = A.weights + r.w;
  const bool both = r.kind == BM_GLCM && A.symmetric;
  const int end = r.cell0 + r.ncell;
  for (int c = r.cell0 + (int)threadIdx.x; c < end; c += PRAD_BM_THREADS) {
    double acc = 0.0;
    if (live) {
      const double *p = M + (long long)c * r.na;
      const int i = c / r.nj, j = c - i * r.nj;
      const double *q = M + (long long)(both ? j * r.nj + i : c) * r.na;      // (read only when `both`)
      acc = bm_weighted_sum(p, q, w, r.na, both);
    }
    o[c] = acc;
  }
}

}  // namespace prad
