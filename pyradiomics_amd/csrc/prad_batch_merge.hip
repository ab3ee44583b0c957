// prad_batch_merge.hip -- C ABI of the weighted angle merge of the batched small-ROI route (include/pyradiomics_amd.h:
// prad_batch_merge_plan[_ng], prad_batch_merge_angles[_ng]_dev); translation unit of libpyradiomics_amd.so.  One implementation, on
// a grey-level count per ROI (RoiLevels): the _ng entry points hand it their vector, the scalar ones one count for all.
#include "kernels_batch_merge.h"
#include "prad_batch_common.h"

#include <algorithm>

using namespace prad;

namespace {

struct MergeLayout {
  std::vector<long long> offsets;   // [3][B + 1]: merged GLCM, merged GLRLM, weights
  long long nrec = 0;
};

inline long long cells_of(int f, const int *sz, int Ng) {
  return f == BM_GLCM ? (long long)Ng * Ng : (long long)Ng * std::max(sz[0], std::max(sz[1], sz[2]));
}

// Host only: no device is touched.
int merge_layout(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, MergeLayout *lay) {
  PRAD_TRY(roi_count_check("batch merge", sizes, B, 0));
  if (B > 0 && !Na) return fail(PRAD_E_ARG, "batch merge: Na is NULL");
  PRAD_TRY(roi_levels_check("batch merge", Ng, B));
  if (families < 1 || (families & ~(PRAD_BATCH_GLCM | PRAD_BATCH_GLRLM)))
    return fail(PRAD_E_ARG, "batch merge: families=%d is no subset of GLCM | GLRLM", families);
  PRAD_TRY(roi_sizes_check("batch merge", sizes, B, nullptr));
  lay->offsets.assign((size_t)3 * (B + 1), 0);
  long long *o = lay->offsets.data();
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    if (Na[b] < 0 || Na[(size_t)B + b] < 0) return fail(PRAD_E_ARG, "batch merge: negative angle count of ROI %d", b);
    for (int f = 0; f < 2; f++) {
      const long long cells = (families >> f) & 1 ? cells_of(f, sz, Ng[b]) : 0;
      if (cells > 0x7fffffffLL) return fail(PRAD_E_UNSUPPORTED, "batch merge: ROI %d has %lld cells", b, cells);
      o[(size_t)f * (B + 1) + b + 1] = o[(size_t)f * (B + 1) + b] + cells;
      lay->nrec += (cells + PRAD_BM_CELLS - 1) / PRAD_BM_CELLS;
    }
    o[(size_t)2 * (B + 1) + b + 1] = o[(size_t)2 * (B + 1) + b] + Na[b] + Na[(size_t)B + b];
  }
  return PRAD_OK;
}

int merge_plan(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, long long *out_offsets);
int merge_angles(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const double *glcm, const double *glrlm,
                 const long long *offsets, const double *weights, const int *status, int symmetric, double *glcm_w,
                 double *glrlm_w, void *stream);

}  // namespace

extern "C" int prad_batch_merge_plan(const int *sizes, int B, int Ng, int families, const int *Na, long long *out_offsets) {
  return merge_plan(sizes, B, RoiLevels{nullptr, Ng}, families, Na, out_offsets);
}

extern "C" int prad_batch_merge_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *Na,
                                        long long *out_offsets) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch merge plan: Ng is NULL");
  return merge_plan(sizes, B, RoiLevels{Ng, 1}, families, Na, out_offsets);
}

extern "C" int prad_batch_merge_angles_dev(const int *sizes, int B, int Ng, int families, const int *Na, const double *glcm,
                                           const double *glrlm, const long long *offsets, const double *weights,
                                           const int *status, int symmetric, double *glcm_w, double *glrlm_w, void *stream) {
  return merge_angles(sizes, B, RoiLevels{nullptr, Ng}, families, Na, glcm, glrlm, offsets, weights, status, symmetric, glcm_w,
                      glrlm_w, stream);
}

extern "C" int prad_batch_merge_angles_ng_dev(const int *sizes, int B, const int *Ng, int families, const int *Na,
                                              const double *glcm, const double *glrlm, const long long *offsets,
                                              const double *weights, const int *status, int symmetric, double *glcm_w,
                                              double *glrlm_w, void *stream) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch merge: Ng is NULL");
  return merge_angles(sizes, B, RoiLevels{Ng, 1}, families, Na, glcm, glrlm, offsets, weights, status, symmetric, glcm_w, glrlm_w,
                      stream);
}

namespace {

int merge_plan(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, long long *out_offsets) {
  if (!out_offsets) return fail(PRAD_E_ARG, "batch merge plan: NULL output");
  MergeLayout lay;
  PRAD_TRY(merge_layout(sizes, B, Ng, families, Na, &lay));
  std::copy(lay.offsets.begin(), lay.offsets.end(), out_offsets);
  return PRAD_OK;
}

int merge_angles(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const double *glcm, const double *glrlm,
                 const long long *offsets, const double *weights, const int *status, int symmetric, double *glcm_w,
                 double *glrlm_w, void *stream) {
  MergeLayout lay;
  PRAD_TRY(merge_layout(sizes, B, Ng, families, Na, &lay));
  if (B == 0 || lay.nrec == 0) return PRAD_OK;
  if (lay.nrec > 0x7fffffffLL) return fail(PRAD_E_UNSUPPORTED, "batch merge: %lld records", lay.nrec);
  const double *in[2] = {glcm, glrlm};
  double *out[2] = {glcm_w, glrlm_w};
  const long long *o = lay.offsets.data();
  const long long nw = o[(size_t)2 * (B + 1) + B];
  if (!offsets || (nw > 0 && !weights)) return fail(PRAD_E_ARG, "batch merge: NULL offsets or weights");
  for (int f = 0; f < 2; f++) {
    if (!((families >> f) & 1)) continue;
    if (!out[f]) return fail(PRAD_E_ARG, "batch merge: merged buffer %d is NULL", f);
    for (int b = 0; b < B; b++) {
      if (offsets[(size_t)f * (B + 1) + b] < 0) return fail(PRAD_E_ARG, "batch merge: negative offset of ROI %d, family %d", b, f);
      if (Na[(size_t)f * B + b] > 0 && !in[f]) return fail(PRAD_E_ARG, "batch merge: matrices of family %d are NULL", f);
    }
  }
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  // ---- the record table, ROI by ROI, and the weights behind it: one upload ------------------------------------------------------
  RecordTable<BatchMergeRec> table;
  PRAD_TRY(table.reserve(c, "batch_merge_meta", (size_t)lay.nrec, sizeof(double) * (size_t)std::max(nw, 1LL)));
  BatchMergeRec *recs = table.host;
  std::copy(weights, weights + nw, (double *)table.host_tail());
  size_t k = 0;
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    for (int f = 0; f < 2; f++) {
      if (!((families >> f) & 1)) continue;
      const long long cells = cells_of(f, sz, Ng[b]);
      for (long long c0 = 0; c0 < cells; c0 += PRAD_BM_CELLS) {
        BatchMergeRec &r = recs[k++];
        r.in = offsets[(size_t)f * (B + 1) + b];
        r.out = o[(size_t)f * (B + 1) + b];
        r.w = o[(size_t)2 * (B + 1) + b] + (f == BM_GLRLM ? Na[b] : 0);
        r.cell0 = (int)c0;
        r.ncell = (int)std::min<long long>(PRAD_BM_CELLS, cells - c0);
        r.nj = (int)(cells / Ng[b]);
        r.na = Na[(size_t)f * B + b];
        r.kind = f, r.roi = b;
      }
    }
  }
  if ((long long)k != lay.nrec) return fail(PRAD_E_ARG, "batch merge: %zu records laid out, %lld planned", k, lay.nrec);

  BatchMergeArgs A;
  A.recs = table.dev;
  A.glcm = glcm, A.glrlm = glrlm;
  A.weights = (const double *)table.dev_tail();
  A.status = status;
  A.glcm_w = glcm_w, A.glrlm_w = glrlm_w;
  A.symmetric = symmetric ? 1 : 0;
  return batch_call(c, s, table, "batch-merge", [&]() {
    Timed t(c, "batch_merge", s);
    hipLaunchKernelGGL(batch_merge_kernel, dim3((unsigned)lay.nrec), dim3(PRAD_BM_THREADS), 0, s, A);
    return check_launch("batch_merge_kernel");
  });
}

}  // namespace
