// prad_batch_features.hip -- C ABI of the batched feature formulas (include/pyradiomics_amd.h: prad_batch_features_plan,
// prad_batch_features_plan_ng, prad_batch_features[_ng]_dev); translation unit of libpyradiomics_amd.so.  One implementation, on a
// grey-level count per ROI (RoiLevels): the _ng entry points hand it their vector, the scalar ones one count for all.
#include "kernels_batch_features.h"
#include "prad_batch_common.h"

#include <algorithm>

using namespace prad;

namespace {

const int kRow[BF_KINDS] = {PRAD_BF_GLCM_ROW, ZM_COUNT, ZM_COUNT, 5, ZM_COUNT};

struct FeatLayout {
  std::vector<long long> offsets;   // [2][5][B + 1]: first double of out, first row (= empty flag)
  long long nrec = 0, nglcm = 0, scratch = 0;
  bool in_domain = true;
  char why[96] = {0};
};

// rows of ROI b in family f
inline int rows_of(int f, int b, int B, const int *Na) { return f == BF_GLCM ? Na[b] : (f == BF_GLRLM ? Na[(size_t)B + b] : 1); }
inline bool has_glszm(const int *glszm_cols, int b) { return glszm_cols[b] >= 1; }

// Host only: no device is touched.
int features_layout(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const int *glszm_cols, FeatLayout *lay) {
  if (B < 0 || (B > 0 && (!sizes || !Na))) return fail(PRAD_E_ARG, "batch features: B=%d, sizes=%p, Na=%p", B, (const void *)sizes, (const void *)Na);
  PRAD_TRY(roi_levels_check("batch features", Ng, B));
  if (families < 1 || families > PRAD_BATCH_FEATURES_ALL) return fail(PRAD_E_ARG, "batch features: families=%d outside [1, %d]", families, PRAD_BATCH_FEATURES_ALL);
  if ((families & PRAD_BATCH_GLSZM) && B > 0 && !glszm_cols) return fail(PRAD_E_ARG, "batch features: GLSZM without its column counts");
  for (int b = 0; b < B; b++) {
    for (int d = 0; d < 3; d++)
      if (sizes[3 * b + d] < 1) return fail(PRAD_E_ARG, "batch features: ROI %d has size[%d]=%d < 1", b, d, sizes[3 * b + d]);
    if (Na[b] < 0 || Na[(size_t)B + b] < 0) return fail(PRAD_E_ARG, "batch features: negative angle count of ROI %d", b);
  }
  lay->in_domain = !roi_levels_above(Ng, B, PRAD_BF_MAX_NG, lay->why, sizeof(lay->why));
  lay->offsets.assign((size_t)2 * BF_KINDS * (B + 1), 0);
  long long *el = lay->offsets.data(), *row = el + (size_t)BF_KINDS * (B + 1);
  long long e = 0, r = 0;
  for (int f = 0; f < BF_KINDS; f++) {
    const bool on = (families >> f) & 1;
    for (int b = 0; b <= B; b++) {
      el[(size_t)f * (B + 1) + b] = e;
      row[(size_t)f * (B + 1) + b] = r;
      if (b == B || !on) continue;
      const int n = rows_of(f, b, B, Na);
      e += (long long)n * kRow[f];
      r += n;
      const bool rec = f != BF_GLSZM || has_glszm(glszm_cols, b);      // (a GLSZM the caller evaluates keeps its row)
      if (rec) lay->nrec += n;
      if (f == BF_GLCM) lay->nglcm += n;
      const int *sz = sizes + 3 * b;
      const long long nj = f == BF_GLRLM ? std::max(sz[0], std::max(sz[1], sz[2])) : (f == BF_GLDM ? 4LL * Na[b] + 1 : (f == BF_GLSZM ? glszm_cols[b] : 0));
      if (rec && (f == BF_GLRLM || f == BF_GLDM || f == BF_GLSZM)) lay->scratch += (long long)n * (Ng[b] + nj);
    }
  }
  return PRAD_OK;
}

int features_plan(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const int *glszm_cols,
                  long long *out_offsets, long long *nrec);
int features_dev(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const int *glszm_cols, const double *glcm,
                 const double *glrlm, const double *gldm, const double *ngtdm, const long long *offsets, const double *glszm,
                 const long long *glszm_offsets, const int *glszm_sizes, const long long *glszm_sizes_offsets, int symmetric,
                 int want_mcc, double *out, int *empty, void *stream);

}  // namespace

extern "C" int prad_batch_features_plan(const int *sizes, int B, int Ng, int families, const int *Na, const int *glszm_cols,
                                        long long *out_offsets, long long *nrec) {
  return features_plan(sizes, B, RoiLevels{nullptr, Ng}, families, Na, glszm_cols, out_offsets, nrec);
}

extern "C" int prad_batch_features_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *Na,
                                           const int *glszm_cols, long long *out_offsets, long long *nrec) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch features plan: Ng is NULL");
  return features_plan(sizes, B, RoiLevels{Ng, 1}, families, Na, glszm_cols, out_offsets, nrec);
}

extern "C" int prad_batch_features_dev(const int *sizes, int B, int Ng, int families, const int *Na, const int *glszm_cols,
                                       const double *glcm, const double *glrlm, const double *gldm, const double *ngtdm,
                                       const long long *offsets, const double *glszm, const long long *glszm_offsets,
                                       const int *glszm_sizes, const long long *glszm_sizes_offsets, int symmetric,
                                       int want_mcc, double *out, int *empty, void *stream) {
  return features_dev(sizes, B, RoiLevels{nullptr, Ng}, families, Na, glszm_cols, glcm, glrlm, gldm, ngtdm, offsets, glszm,
                      glszm_offsets, glszm_sizes, glszm_sizes_offsets, symmetric, want_mcc, out, empty, stream);
}

extern "C" int prad_batch_features_ng_dev(const int *sizes, int B, const int *Ng, int families, const int *Na,
                                          const int *glszm_cols, const double *glcm, const double *glrlm, const double *gldm,
                                          const double *ngtdm, const long long *offsets, const double *glszm,
                                          const long long *glszm_offsets, const int *glszm_sizes,
                                          const long long *glszm_sizes_offsets, int symmetric, int want_mcc, double *out,
                                          int *empty, void *stream) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch features: Ng is NULL");
  return features_dev(sizes, B, RoiLevels{Ng, 1}, families, Na, glszm_cols, glcm, glrlm, gldm, ngtdm, offsets, glszm, glszm_offsets,
                      glszm_sizes, glszm_sizes_offsets, symmetric, want_mcc, out, empty, stream);
}

namespace {

int features_plan(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const int *glszm_cols,
                  long long *out_offsets, long long *nrec) {
  if (!out_offsets || !nrec) return fail(PRAD_E_ARG, "batch features plan: NULL output");
  FeatLayout lay;
  PRAD_TRY(features_layout(sizes, B, Ng, families, Na, glszm_cols, &lay));
  std::copy(lay.offsets.begin(), lay.offsets.end(), out_offsets);
  nrec[0] = lay.nrec, nrec[1] = lay.nglcm, nrec[2] = lay.scratch;
  if (!lay.in_domain) return fail(PRAD_E_UNSUPPORTED, "batch features: %s (use the single calls per ROI)", lay.why);
  return PRAD_OK;
}

int features_dev(const int *sizes, int B, const RoiLevels &Ng, int families, const int *Na, const int *glszm_cols, const double *glcm,
                 const double *glrlm, const double *gldm, const double *ngtdm, const long long *offsets, const double *glszm,
                 const long long *glszm_offsets, const int *glszm_sizes, const long long *glszm_sizes_offsets, int symmetric,
                 int want_mcc, double *out, int *empty, void *stream) {
  FeatLayout lay;
  PRAD_TRY(features_layout(sizes, B, Ng, families, Na, glszm_cols, &lay));
  if (!lay.in_domain) return fail(PRAD_E_UNSUPPORTED, "batch features: %s (use the single calls per ROI)", lay.why);   // nothing launched
  if (B == 0 || lay.nrec == 0) return PRAD_OK;
  const double *mats[BF_KINDS] = {glcm, glrlm, gldm, ngtdm, glszm};
  if (!out || !empty) return fail(PRAD_E_ARG, "batch features: NULL output");
  if ((families & PRAD_BATCH_ALL) && !offsets) return fail(PRAD_E_ARG, "batch features: NULL offsets");
  if ((families & PRAD_BATCH_GLSZM) && !glszm_offsets) return fail(PRAD_E_ARG, "batch features: NULL GLSZM offsets");
  if (glszm_sizes && !glszm_sizes_offsets) return fail(PRAD_E_ARG, "batch features: size lists without their offsets");
  if (lay.nrec > 0x7fffffffLL || lay.offsets.back() > 0x7fffffffLL) return fail(PRAD_E_UNSUPPORTED, "batch features: %lld records", lay.nrec);
  const long long *el = lay.offsets.data(), *row = el + (size_t)BF_KINDS * (B + 1);

  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  RecordTable<BatchFeatRec> table;
  double *d_scr = nullptr;
  int *d_flag = nullptr;
  PRAD_TRY(table.reserve(c, "batch_feat_meta", (size_t)lay.nrec));
  PRAD_TRY(c.get<double>("batch_feat_scratch", (size_t)std::max(lay.scratch, 1LL), &d_scr));
  PRAD_TRY(c.get<int>("batch_feat_flag", 4, &d_flag));

  // ---- the record table: GLCM angles first (the MCC launch runs over them alone), then family by family, ROI by ROI ----------
  BatchFeatRec *recs = table.host;
  size_t k = 0;
  long long scr = 0;
  for (int f = 0; f < BF_KINDS; f++) {
    if (!((families >> f) & 1)) continue;
    for (int b = 0; b < B; b++) {
      const int n = rows_of(f, b, B, Na);
      if (n == 0 || (f == BF_GLSZM && !has_glszm(glszm_cols, b))) continue;
      if (!mats[f]) return fail(PRAD_E_ARG, "batch features: matrices of family %d are NULL", f);
      const long long mat = f == BF_GLSZM ? glszm_offsets[b] : offsets[(size_t)f * (B + 1) + b];
      if (mat < 0) return fail(PRAD_E_ARG, "batch features: negative offset of ROI %d, family %d", b, f);
      const int *sz = sizes + 3 * b;
      const int ng = Ng[b];
      int Nj = ng, NaM = 1;
      if (f == BF_GLCM) NaM = n;
      else if (f == BF_GLRLM) Nj = std::max(sz[0], std::max(sz[1], sz[2])), NaM = n;
      else if (f == BF_GLDM) Nj = 4 * Na[b] + 1;
      else if (f == BF_NGTDM) Nj = 3;
      else Nj = glszm_cols[b];
      const bool zone = f == BF_GLRLM || f == BF_GLDM || f == BF_GLSZM;
      for (int a = 0; a < n; a++) {
        BatchFeatRec &r = recs[k++];
        r.mat = mat;
        r.scratch = zone ? scr : 0;
        if (zone) scr += (long long)ng + Nj;
        r.out = el[(size_t)f * (B + 1) + b] + (long long)a * kRow[f];
        r.sizes = (f == BF_GLSZM && glszm_sizes) ? glszm_sizes_offsets[b] : -1;
        r.empty = (int)(row[(size_t)f * (B + 1) + b] + a);
        r.kind = f, r.roi = b, r.a = a;
        r.Ni = ng, r.Nj = Nj, r.Na = NaM, r.pad = 0;
      }
    }
  }
  if ((long long)k != lay.nrec || scr != lay.scratch) return fail(PRAD_E_ARG, "batch features: %zu records laid out, %lld planned", k, lay.nrec);
  const bool mcc = want_mcc && lay.nglcm > 0;

  BatchFeatArgs A;
  A.recs = table.dev;
  for (int f = 0; f < BF_KINDS; f++) A.mats[f] = mats[f];
  A.sizes = glszm_sizes;
  A.scratch = d_scr;
  A.out = out;
  A.empty = empty;
  A.symmetric = symmetric ? 1 : 0;
  A.mcc = mcc ? 1 : 0;
  const int most = Ng.most(B);      // LDS by the largest count of the batch; a workgroup lays its own out by its record's Ni
  const size_t lds = sizeof(double) * batch_features_lds_doubles(most);
  const size_t mcc_lds = ((mcc_scratch_bytes(most, most) + 15) & ~(size_t)15) + sizeof(double) * (size_t)most * most;   // staged

  return batch_call(c, s, table, "batch-features", [&]() {
    if (mcc) {
      PRAD_HIP(hipMemsetAsync(d_flag, 0, sizeof(int) * 4, s));
      PRAD_TRY(allow_dynamic_lds(&batch_mcc_kernel, mcc_lds));
    }
    Timed t(c, "batch_features", s);
    hipLaunchKernelGGL(batch_features_kernel, dim3((unsigned)lay.nrec), dim3(PRAD_FEAT_THREADS), lds, s, A);
    PRAD_TRY(check_launch("batch_features_kernel"));
    if (!mcc) return (int)PRAD_OK;
    hipLaunchKernelGGL(batch_mcc_kernel, dim3((unsigned)lay.nglcm), dim3(PRAD_MCC_BT), mcc_lds, s, A, d_flag);
    return check_launch("batch_mcc_kernel");
  });
}

}  // namespace
