// prad_batch_glszm.hip -- C ABI of the batched small-ROI GLSZM (include/pyradiomics_amd.h: prad_batch_glszm_max_vox,
// prad_batch_glszm[_f2d | _ng]_dev, prad_batch_glszm_fill[_ng]_dev); translation unit of libpyradiomics_amd.so.  One implementation,
// on a grey-level count per ROI (RoiLevels): the _ng entry points hand it their vector, the scalar ones one count for all.
#include "kernels_batch_glszm.h"
#include "prad_batch_common.h"

#include <algorithm>

using namespace prad;

extern "C" int prad_batch_glszm_max_vox(void) { return PRAD_BATCH_GLSZM_MAX_VOX; }

namespace {

template <int F2D>
int launch_zones(Context &c, hipStream_t s, int B, size_t lds, const BatchZoneArgs &A) {
  PRAD_TRY(allow_dynamic_lds(&batch_glszm_kernel<F2D>, lds));
  Timed t(c, "batch_glszm", s);
  hipLaunchKernelGGL(batch_glszm_kernel<F2D>, dim3((unsigned)B), dim3(PRAD_BZ_THREADS), lds, s, A);
  return check_launch("batch_glszm_kernel");
}

int batch_glszm(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, const RoiLevels &Ng,
                int force2Ddim, int *zones, int *summary, int *status, void *stream);
int batch_glszm_fill(const int *zones, const int *summary_host, const long long *off, int B, const RoiLevels &Ng, int compact,
                     double *out, const long long *out_offsets, int *sizes_out, const long long *sizes_offsets, void *stream);

}  // namespace

extern "C" int prad_batch_glszm_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                    int Ng, int *zones, int *summary, int *status, void *stream) {
  return prad_batch_glszm_f2d_dev(levels, mask, sizes, off, B, Ng, -1, zones, summary, status, stream);
}

extern "C" int prad_batch_glszm_f2d_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                        int Ng, int force2Ddim, int *zones, int *summary, int *status, void *stream) {
  return batch_glszm(levels, mask, sizes, off, B, RoiLevels{nullptr, Ng}, force2Ddim, zones, summary, status, stream);
}

extern "C" int prad_batch_glszm_ng_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                       const int *Ng, int force2Ddim, int *zones, int *summary, int *status, void *stream) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch GLSZM: Ng is NULL");
  return batch_glszm(levels, mask, sizes, off, B, RoiLevels{Ng, 1}, force2Ddim, zones, summary, status, stream);
}

extern "C" int prad_batch_glszm_fill_dev(const int *zones, const int *summary_host, const long long *off, int B, int Ng,
                                         int compact, double *out, const long long *out_offsets, int *sizes_out,
                                         const long long *sizes_offsets, void *stream) {
  return batch_glszm_fill(zones, summary_host, off, B, RoiLevels{nullptr, Ng}, compact, out, out_offsets, sizes_out, sizes_offsets,
                          stream);
}

extern "C" int prad_batch_glszm_fill_ng_dev(const int *zones, const int *summary_host, const long long *off, int B, const int *Ng,
                                            int compact, double *out, const long long *out_offsets, int *sizes_out,
                                            const long long *sizes_offsets, void *stream) {
  if (B > 0 && !Ng) return fail(PRAD_E_ARG, "batch GLSZM fill: Ng is NULL");
  return batch_glszm_fill(zones, summary_host, off, B, RoiLevels{Ng, 1}, compact, out, out_offsets, sizes_out, sizes_offsets, stream);
}

namespace {

int batch_glszm(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B, const RoiLevels &Ng,
                int force2Ddim, int *zones, int *summary, int *status, void *stream) {
  PRAD_TRY(roi_count_check("batch GLSZM", sizes, B, 0));
  PRAD_TRY(roi_levels_check("batch GLSZM", Ng, B));
  if (force2Ddim < -1 || force2Ddim > 2) return fail(PRAD_E_ARG, "batch GLSZM: forced dimension %d outside [-1, 2]", force2Ddim);
  long long max_vox = 1;
  PRAD_TRY(roi_sizes_check("batch GLSZM", sizes, B, &max_vox));
  if (B > 0 && (!levels || !mask || !off || !zones || !summary || !status)) return fail(PRAD_E_ARG, "batch GLSZM: NULL pointer");
  PRAD_TRY(roi_offsets_check("batch GLSZM", off, B));
  // valid arguments outside the domain: nothing is launched
  char why[96];
  if (roi_levels_above(Ng, B, PRAD_BZ_MAX_NG, why, sizeof(why))) return fail(PRAD_E_UNSUPPORTED, "batch GLSZM: %s (use the single call per ROI)", why);
  for (int b = 0; b < B; b++)
    if (roi_nvox(sizes, b) > PRAD_BATCH_GLSZM_MAX_VOX)
      return fail(PRAD_E_UNSUPPORTED, "batch GLSZM: ROI %d holds %lld voxels, above %d (use the single call per ROI)", b,
                  roi_nvox(sizes, b), PRAD_BATCH_GLSZM_MAX_VOX);
  if (B == 0) return PRAD_OK;
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  RecordTable<BatchZoneRoi> table;
  PRAD_TRY(table.reserve(c, "batch_glszm_meta", (size_t)B));
  BatchZoneRoi *rois = table.host;
  for (int b = 0; b < B; b++) {
    rois[b].off = off[b];
    rois[b].nz = sizes[3 * b], rois[b].ny = sizes[3 * b + 1], rois[b].nx = sizes[3 * b + 2];
    rois[b].Ng = Ng[b];
  }
  BatchZoneArgs A;
  A.levels = levels;
  A.mask = mask;
  A.rois = table.dev;
  A.vox_bytes = (int)((max_vox + 15) & ~15LL);
  A.zones = zones;
  A.summary = summary;
  A.status = status;
  const size_t lds = PRAD_BZ_MISC_BYTES + 3 * (size_t)A.vox_bytes;
  if (lds > 160 * 1024) return fail(PRAD_E_HIP, "batch GLSZM: %zu bytes of LDS per workgroup", lds);

  static const char *const kVariant[4] = {"batch-glszm-lds", "batch-glszm-lds-f2d0", "batch-glszm-lds-f2d1", "batch-glszm-lds-f2d2"};
  return batch_call(c, s, table, kVariant[force2Ddim + 1], [&]() {
    switch (force2Ddim) {
      case 0: return launch_zones<0>(c, s, B, lds, A);
      case 1: return launch_zones<1>(c, s, B, lds, A);
      case 2: return launch_zones<2>(c, s, B, lds, A);
      default: return launch_zones<-1>(c, s, B, lds, A);
    }
  });
}

int batch_glszm_fill(const int *zones, const int *summary_host, const long long *off, int B, const RoiLevels &Ng, int compact,
                     double *out, const long long *out_offsets, int *sizes_out, const long long *sizes_offsets, void *stream) {
  if (B < 0) return fail(PRAD_E_ARG, "batch GLSZM fill: B=%d", B);
  PRAD_TRY(roi_levels_check("batch GLSZM fill", Ng, B));
  if (B > 0 && (!zones || !summary_host || !off || !out || !out_offsets || (compact && (!sizes_out || !sizes_offsets))))
    return fail(PRAD_E_ARG, "batch GLSZM fill: NULL pointer");
  for (int b = 0; b < B; b++) {
    const int *sm = summary_host + 3 * b;
    if (off[b] < 0 || out_offsets[b] < 0 || (compact && sizes_offsets[b] < 0))
      return fail(PRAD_E_ARG, "batch GLSZM fill: negative offset of ROI %d", b);
    if (sm[0] < 0 || sm[1] < 0 || sm[1] > PRAD_BATCH_GLSZM_MAX_VOX || sm[2] < 0 || sm[2] > sm[1] || sm[0] > PRAD_BATCH_GLSZM_MAX_VOX)
      return fail(PRAD_E_ARG, "batch GLSZM fill: summary of ROI %d is (%d, %d, %d)", b, sm[0], sm[1], sm[2]);
  }
  char why[96];
  if (roi_levels_above(Ng, B, PRAD_BZ_MAX_NG, why, sizeof(why))) return fail(PRAD_E_UNSUPPORTED, "batch GLSZM fill: %s", why);
  if (B == 0) return PRAD_OK;
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  RecordTable<BatchFillRoi> table;
  PRAD_TRY(table.reserve(c, "batch_glszm_fill_meta", (size_t)B));
  BatchFillRoi *rois = table.host;
  for (int b = 0; b < B; b++) {
    rois[b].zones = 2 * off[b];
    rois[b].out = out_offsets[b];
    rois[b].sizes = compact ? sizes_offsets[b] : 0;
    rois[b].nzones = summary_host[3 * b];
    rois[b].max_region = summary_host[3 * b + 1];
    rois[b].nsizes = summary_host[3 * b + 2];
    rois[b].Ng = Ng[b];
  }
  return batch_call(c, s, table, "batch-glszm-lds", [&]() {
    Timed t(c, "batch_glszm", s);
    hipLaunchKernelGGL(batch_glszm_fill_kernel, dim3((unsigned)B), dim3(PRAD_BZ_THREADS), 0, s, zones, table.dev, compact ? 1 : 0,
                       out, sizes_out);
    return check_launch("batch_glszm_fill_kernel");
  });
}

}  // namespace
