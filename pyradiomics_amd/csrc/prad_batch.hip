// prad_batch.hip -- C ABI of the batched small-ROI texture matrices (include/pyradiomics_amd.h: prad_batch_plan[_f2d | _ng],
// prad_calculate_batch[_f2d | _ng]_dev); translation unit of libpyradiomics_amd.so.  One implementation, on a grey-level count per
// ROI (RoiLevels): the _ng entry points hand it their vector, the scalar ones one count for all.  The kernel consumes an
// arbitrary angle table per ROI, so the forced dimension (force2D) lives here alone: the counts and tables come from
// prad_get_angle_count / prad_build_angles with it, the very functions the single calls use.
#include "kernels_batch.h"
#include "prad_batch_common.h"

#include <algorithm>

using namespace prad;

namespace {

const int kOne = 1;

struct BatchLayout {
  std::vector<long long> offsets;   // [4][B + 1]
  std::vector<int> na;              // [2][B]: requested distances, distance 1
  bool in_domain = true;
  char why[160] = {0};
};

// Shapes of the per-ROI outputs, the same arithmetic the single calls use: Na = prad_get_angle_count (unidirectional, forced
// dimension f2d: -1 none, 0 / 1 / 2 the axis no angle may leave),
// GLCM [Ng][Ng][Na], GLRLM [Ng][max(size)][Na1] (distance 1), GLDM [Ng][2 Nb + 1] with Nb = 2 Na, NGTDM [Ng][3], Ng the ROI's own.
// Host only: no device is touched.
int batch_layout(const int *sizes, int B, const RoiLevels &Ng, int families, const int *distances, int Ndist, int f2d, BatchLayout *lay) {
  PRAD_TRY(roi_count_check("batch", sizes, B, 0));
  PRAD_TRY(roi_levels_check("batch", Ng, B));
  if (!distances || Ndist < 1) return fail(PRAD_E_ARG, "batch: no distances");
  if (families < 1 || families > PRAD_BATCH_ALL) return fail(PRAD_E_ARG, "batch: families=%d outside [1, %d]", families, PRAD_BATCH_ALL);
  for (int k = 0; k < Ndist; k++)
    if (distances[k] < 1) return fail(PRAD_E_ARG, "batch: distance %d < 1", distances[k]);
  if (f2d < -1 || f2d > 2) return fail(PRAD_E_ARG, "batch: forced dimension %d outside [-1, 2]", f2d);
  PRAD_TRY(roi_sizes_check("batch", sizes, B, nullptr));
  lay->offsets.assign((size_t)4 * (B + 1), 0);
  lay->na.assign((size_t)2 * B, 0);
  if (roi_levels_above(Ng, B, PRAD_BATCH_MAX_NG, lay->why, sizeof(lay->why))) lay->in_domain = false;
  long long *o = lay->offsets.data();
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    const long long nvox = roi_nvox(sizes, b);
    const int na = prad_get_angle_count(sz, distances, 3, Ndist, 0, f2d);
    const int na1 = prad_get_angle_count(sz, &kOne, 3, 1, 0, f2d);
    lay->na[b] = na;
    lay->na[(size_t)B + b] = na1;
    if (lay->in_domain && nvox > PRAD_BATCH_MAX_VOX) {
      lay->in_domain = false;
      snprintf(lay->why, sizeof(lay->why), "ROI %d holds %lld voxels, above %d", b, nvox, PRAD_BATCH_MAX_VOX);
    }
    if (lay->in_domain && na > PRAD_BATCH_MAX_NA) {
      lay->in_domain = false;
      snprintf(lay->why, sizeof(lay->why), "ROI %d has %d angles, above %d", b, na, PRAD_BATCH_MAX_NA);
    }
    const long long Nr = std::max(sz[0], std::max(sz[1], sz[2])), ng = Ng[b];
    const long long per[4] = {ng * ng * na, ng * Nr * na1, ng * (4 * na + 1), ng * 3};
    for (int f = 0; f < 4; f++)
      o[(size_t)f * (B + 1) + b + 1] = o[(size_t)f * (B + 1) + b] + ((families >> f) & 1 ? per[f] : 0);
  }
  return PRAD_OK;
}

int batch_plan(const int *sizes, int B, const RoiLevels &Ng, int families, const int *distances, int Ndist, int force2Ddim,
               long long *out_offsets, int *Na) {
  if (!out_offsets || !Na) return fail(PRAD_E_ARG, "batch plan: NULL output");
  BatchLayout lay;
  PRAD_TRY(batch_layout(sizes, B, Ng, families, distances, Ndist, force2Ddim, &lay));
  std::copy(lay.offsets.begin(), lay.offsets.end(), out_offsets);
  std::copy(lay.na.begin(), lay.na.end(), Na);
  if (!lay.in_domain) return fail(PRAD_E_UNSUPPORTED, "batch: %s (use the single calls per ROI)", lay.why);
  return PRAD_OK;
}

int calculate_batch(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, const RoiLevels &Ng,
                    int families, const int *distances, int Ndist, int alpha, int force2Ddim, double *glcm, double *glrlm,
                    double *gldm, double *ngtdm, int *status, void *stream);

}  // namespace

extern "C" int prad_batch_max_vox(void) { return PRAD_BATCH_MAX_VOX; }

extern "C" int prad_batch_plan(const int *sizes, int B, int Ng, int families, const int *distances, int Ndist,
                               long long *out_offsets, int *Na) {
  return prad_batch_plan_f2d(sizes, B, Ng, families, distances, Ndist, -1, out_offsets, Na);
}

extern "C" int prad_batch_plan_f2d(const int *sizes, int B, int Ng, int families, const int *distances, int Ndist,
                                   int force2Ddim, long long *out_offsets, int *Na) {
  return batch_plan(sizes, B, RoiLevels{nullptr, Ng}, families, distances, Ndist, force2Ddim, out_offsets, Na);
}

extern "C" int prad_batch_plan_ng(const int *sizes, int B, const int *Ng, int families, const int *distances, int Ndist,
                                  int force2Ddim, long long *out_offsets, int *Na) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch plan: Ng is NULL");
  return batch_plan(sizes, B, RoiLevels{Ng, 1}, families, distances, Ndist, force2Ddim, out_offsets, Na);
}

extern "C" int prad_calculate_batch_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off,
                                        int B, int Ng, int families, const int *distances, int Ndist, int alpha,
                                        double *glcm, double *glrlm, double *gldm, double *ngtdm, int *status,
                                        void *stream) {
  return prad_calculate_batch_f2d_dev(levels, mask, sizes, off, B, Ng, families, distances, Ndist, alpha, -1, glcm, glrlm, gldm,
                                      ngtdm, status, stream);
}

extern "C" int prad_calculate_batch_f2d_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off,
                                            int B, int Ng, int families, const int *distances, int Ndist, int alpha,
                                            int force2Ddim, double *glcm, double *glrlm, double *gldm, double *ngtdm,
                                            int *status, void *stream) {
  return calculate_batch(levels, mask, sizes, off, B, RoiLevels{nullptr, Ng}, families, distances, Ndist, alpha, force2Ddim, glcm,
                         glrlm, gldm, ngtdm, status, stream);
}

extern "C" int prad_calculate_batch_ng_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off,
                                           int B, const int *Ng, int families, const int *distances, int Ndist, int alpha,
                                           int force2Ddim, double *glcm, double *glrlm, double *gldm, double *ngtdm,
                                           int *status, void *stream) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch: Ng is NULL");
  return calculate_batch(levels, mask, sizes, off, B, RoiLevels{Ng, 1}, families, distances, Ndist, alpha, force2Ddim, glcm, glrlm,
                         gldm, ngtdm, status, stream);
}

namespace {

int calculate_batch(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, const RoiLevels &Ng,
                    int families, const int *distances, int Ndist, int alpha, int force2Ddim, double *glcm, double *glrlm,
                    double *gldm, double *ngtdm, int *status, void *stream) {
  BatchLayout lay;
  PRAD_TRY(batch_layout(sizes, B, Ng, families, distances, Ndist, force2Ddim, &lay));
  if (!lay.in_domain) return fail(PRAD_E_UNSUPPORTED, "batch: %s (use the single calls per ROI)", lay.why);   // nothing launched
  if (B == 0) return PRAD_OK;
  double *outs[4] = {glcm, glrlm, gldm, ngtdm};
  for (int f = 0; f < 4; f++) {
    if (!((families >> f) & 1)) outs[f] = nullptr;
    else if (!outs[f] && lay.offsets[(size_t)f * (B + 1) + B] > 0) return fail(PRAD_E_ARG, "batch: output %d is NULL", f);
  }
  if (!levels || !mask || !off || !status) return fail(PRAD_E_ARG, "batch: NULL pointer");
  if (alpha < 0) return fail(PRAD_E_ARG, "batch: alpha=%d < 0", alpha);
  PRAD_TRY(roi_offsets_check("batch", off, B));
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  // ---- per-ROI records and the concatenated angle tables (prad_build_angles), one upload -----------------------------------
  const bool runs = (families & PRAD_BATCH_GLRLM) != 0, same = Ndist == 1 && distances[0] == 1;
  size_t nang = 0;
  for (int b = 0; b < B; b++) nang += (size_t)lay.na[b] + (runs && !same ? (size_t)lay.na[(size_t)B + b] : 0);
  RecordTable<BatchRoi> table;
  PRAD_TRY(table.reserve(c, "batch_meta", (size_t)B, sizeof(int) * 3 * std::max<size_t>(nang, 1)));
  BatchRoi *rois = table.host;
  int *angles = (int *)table.host_tail();
  long long max_vox = 1;
  // table region, the most any ROI asks for with its own Ng: up to PRAD_BATCH_ANGLES_AT_ONCE angles of GLCM / GLRLM at once,
  // every level of GLDM + NGTDM; and the least every ROI needs: one GLCM angle (hence one GLRLM column per level), one level
  // of GLDM + NGTDM
  long long want[3] = {0, 0, 0}, floor_words = 1;
  size_t row = 0;
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    BatchRoi &r = rois[b];
    r.off = off[b];
    for (int f = 0; f < 4; f++) r.out[f] = lay.offsets[(size_t)f * (B + 1) + b];
    r.nz = sz[0], r.ny = sz[1], r.nx = sz[2];
    r.na = lay.na[b];
    r.na_run = lay.na[(size_t)B + b];
    r.Ng = Ng[b];
    r.ang = (int)row;
    if (r.na > 0 && prad_build_angles(sz, distances, 3, Ndist, force2Ddim, r.na, angles + 3 * row) != 0)
      return fail(PRAD_E_ARG, "batch: angles of ROI %d", b);
    row += (size_t)r.na;
    r.ang_run = r.ang;
    if (runs && !same) {
      r.ang_run = (int)row;
      if (r.na_run > 0 && prad_build_angles(sz, &kOne, 3, 1, force2Ddim, r.na_run, angles + 3 * row) != 0)
        return fail(PRAD_E_ARG, "batch: distance-1 angles of ROI %d", b);
      row += (size_t)r.na_run;
    }
    max_vox = std::max(max_vox, roi_nvox(sizes, b));
    const long long ng = r.Ng, nr = std::max(sz[0], std::max(sz[1], sz[2])), W = 2LL * r.na + 1;
    want[0] = std::max(want[0], PRAD_BATCH_ANGLES_AT_ONCE * ng * ng);
    want[1] = std::max(want[1], PRAD_BATCH_ANGLES_AT_ONCE * ng * nr);
    want[2] = std::max(want[2], 2 * W * ng);
    floor_words = std::max(floor_words, std::max(ng * ng, 2 * W));
  }

  // ---- launch geometry ------------------------------------------------------------------------------------------------------
  BatchArgs A;
  A.levels = levels;
  A.mask = mask;
  A.rois = table.dev;
  A.angles = (const int *)table.dev_tail();
  A.alpha = alpha;
  A.glcm = outs[0], A.glrlm = outs[1], A.gldm = outs[2], A.ngtdm = outs[3];
  A.status = status;
  // Angle groups per ROI: every group packs the ROI again, so a large batch takes one group per family (B workgroups fill the
  // card by themselves) and a small one splits its angles until ~2048 workgroups exist (PRAD_BATCH_GROUPS overrides).
  static const int fixed = getenv("PRAD_BATCH_GROUPS") ? atoi(getenv("PRAD_BATCH_GROUPS")) : 0;
  const int pair_fams = (outs[0] ? 1 : 0) + (outs[1] ? 1 : 0);
  int groups = fixed > 0 ? fixed : (int)((2048 + (long long)B * std::max(pair_fams, 1) - 1) / ((long long)B * std::max(pair_fams, 1)));
  groups = std::max(1, std::min(groups, 13));
  A.groups_glcm = outs[0] ? groups : 0;
  A.groups_glrlm = outs[1] ? groups : 0;
  A.neigh = (outs[2] || outs[3]) ? 1 : 0;
  if (!A.groups_glcm && !A.groups_glrlm) A.neigh = 1;   // (only empty matrices asked for: a job per ROI still gives its status)
  long long words = 64;
  if (outs[0]) words = std::max(words, want[0]);
  if (outs[1]) words = std::max(words, want[1]);
  if (A.neigh) words = std::max(words, want[2]);
  words = std::min<long long>(words, PRAD_BATCH_TABLE_BYTES / 4);
  words = std::max<long long>(words, floor_words);   // (below the budget: Ng <= 64, Na <= 127)
  A.table_words = (int)words;
  const size_t lds = PRAD_BATCH_MISC_BYTES + 4 * (size_t)words + (((size_t)max_vox + 15) & ~(size_t)15);
  if (lds > 160 * 1024 / 2) return fail(PRAD_E_HIP, "batch: %zu bytes of LDS per workgroup", lds);
  const long long jobs = A.groups_glcm + A.groups_glrlm + A.neigh;
  if ((long long)B * jobs > 0x7fffffffLL) return fail(PRAD_E_UNSUPPORTED, "batch: %d ROIs x %lld jobs", B, jobs);

  return batch_call(c, s, table, force2Ddim < 0 ? "batch-lds" : "batch-lds-f2d", [&]() {
    PRAD_TRY(allow_dynamic_lds(&batch_rois_kernel, lds));
    Timed t(c, "batch", s);
    hipLaunchKernelGGL(batch_rois_kernel, dim3((unsigned)(B * jobs)), dim3(PRAD_BATCH_THREADS), lds, s, A);
    return check_launch("batch_rois_kernel");
  });
}

}  // namespace
