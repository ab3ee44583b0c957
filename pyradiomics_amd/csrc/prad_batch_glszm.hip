// prad_batch_glszm.hip -- C ABI of the batched small-ROI GLSZM (include/pyradiomics_amd.h: prad_batch_glszm_max_vox,
// prad_batch_glszm_dev, prad_batch_glszm_fill_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_glszm.h"

#include <algorithm>

using namespace prad;

namespace {

// Host only: no device is touched.  *why is set (and PRAD_OK returned) when the arguments are valid but outside the domain.
int zone_batch_check(const int *sizes, int B, int Ng, long long *max_vox, char *why, size_t why_len) {
  why[0] = 0;
  *max_vox = 1;
  if (B < 0 || (B > 0 && !sizes)) return fail(PRAD_E_ARG, "batch GLSZM: B=%d, sizes=%p", B, (const void *)sizes);
  if (Ng < 1) return fail(PRAD_E_ARG, "batch GLSZM: Ng=%d < 1", Ng);
  if (Ng > PRAD_BZ_MAX_NG) snprintf(why, why_len, "Ng=%d above %d", Ng, PRAD_BZ_MAX_NG);
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    for (int d = 0; d < 3; d++)
      if (sz[d] < 1) return fail(PRAD_E_ARG, "batch GLSZM: ROI %d has size[%d]=%d < 1", b, d, sz[d]);
    const long long nvox = (long long)sz[0] * sz[1] * sz[2];
    if (!why[0] && nvox > PRAD_BATCH_GLSZM_MAX_VOX)
      snprintf(why, why_len, "ROI %d holds %lld voxels, above %d", b, nvox, PRAD_BATCH_GLSZM_MAX_VOX);
    *max_vox = std::max(*max_vox, nvox);
  }
  return PRAD_OK;
}

}  // namespace

extern "C" int prad_batch_glszm_max_vox(void) { return PRAD_BATCH_GLSZM_MAX_VOX; }

extern "C" int prad_batch_glszm_dev(const int32_t *levels, const uint8_t *mask, const int *sizes, const long long *off, int B,
                                    int Ng, int *zones, int *summary, int *status, void *stream) {
  long long max_vox = 1;
  char why[160];
  PRAD_TRY(zone_batch_check(sizes, B, Ng, &max_vox, why, sizeof(why)));
  if (B > 0 && (!levels || !mask || !off || !zones || !summary || !status)) return fail(PRAD_E_ARG, "batch GLSZM: NULL pointer");
  for (int b = 0; b < B; b++)
    if (off[b] < 0) return fail(PRAD_E_ARG, "batch GLSZM: off[%d]=%lld < 0", b, off[b]);
  if (why[0]) return fail(PRAD_E_UNSUPPORTED, "batch GLSZM: %s (use the single call per ROI)", why);   // nothing launched
  if (B == 0) return PRAD_OK;
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  const size_t meta_bytes = sizeof(BatchZoneRoi) * (size_t)B;
  void *h_meta = nullptr, *d_meta = nullptr;
  PRAD_TRY(c.get_pinned("batch_glszm_meta", meta_bytes, &h_meta));
  PRAD_TRY(c.get("batch_glszm_meta", meta_bytes, &d_meta));
  BatchZoneRoi *rois = (BatchZoneRoi *)h_meta;
  for (int b = 0; b < B; b++) {
    rois[b].off = off[b];
    rois[b].nz = sizes[3 * b], rois[b].ny = sizes[3 * b + 1], rois[b].nx = sizes[3 * b + 2];
    rois[b].pad = 0;
  }
  BatchZoneArgs A;
  A.levels = levels;
  A.mask = mask;
  A.rois = (const BatchZoneRoi *)d_meta;
  A.Ng = Ng;
  A.vox_bytes = (int)((max_vox + 15) & ~15LL);
  A.zones = zones;
  A.summary = summary;
  A.status = status;
  const size_t lds = PRAD_BZ_MISC_BYTES + 3 * (size_t)A.vox_bytes;
  if (lds > 160 * 1024) return fail(PRAD_E_HIP, "batch GLSZM: %zu bytes of LDS per workgroup", lds);

  PRAD_TRY(c.begin_call(s));
  PRAD_HIP(hipMemcpyAsync(d_meta, h_meta, meta_bytes, hipMemcpyHostToDevice, s));
  if (lds > 64 * 1024)
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&batch_glszm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int rc;
  {
    Timed t(c, "batch_glszm", s);
    hipLaunchKernelGGL(batch_glszm_kernel, dim3((unsigned)B), dim3(PRAD_BZ_THREADS), lds, s, A);
    rc = check_launch("batch_glszm_kernel");
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));   // (the pinned record block is reused by the next call)
  c.last_path = "batch";
  c.last_variant = "batch-glszm-lds";
  return PRAD_OK;
}

extern "C" int prad_batch_glszm_fill_dev(const int *zones, const int *summary_host, const long long *off, int B, int Ng,
                                         int compact, double *out, const long long *out_offsets, int *sizes_out,
                                         const long long *sizes_offsets, void *stream) {
  if (B < 0) return fail(PRAD_E_ARG, "batch GLSZM fill: B=%d", B);
  if (Ng < 1) return fail(PRAD_E_ARG, "batch GLSZM fill: Ng=%d < 1", Ng);
  if (B > 0 && (!zones || !summary_host || !off || !out || !out_offsets || (compact && (!sizes_out || !sizes_offsets))))
    return fail(PRAD_E_ARG, "batch GLSZM fill: NULL pointer");
  for (int b = 0; b < B; b++) {
    const int *sm = summary_host + 3 * b;
    if (off[b] < 0 || out_offsets[b] < 0 || (compact && sizes_offsets[b] < 0))
      return fail(PRAD_E_ARG, "batch GLSZM fill: negative offset of ROI %d", b);
    if (sm[0] < 0 || sm[1] < 0 || sm[1] > PRAD_BATCH_GLSZM_MAX_VOX || sm[2] < 0 || sm[2] > sm[1] || sm[0] > PRAD_BATCH_GLSZM_MAX_VOX)
      return fail(PRAD_E_ARG, "batch GLSZM fill: summary of ROI %d is (%d, %d, %d)", b, sm[0], sm[1], sm[2]);
  }
  if (Ng > PRAD_BZ_MAX_NG) return fail(PRAD_E_UNSUPPORTED, "batch GLSZM fill: Ng=%d above %d", Ng, PRAD_BZ_MAX_NG);
  if (B == 0) return PRAD_OK;
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  const size_t meta_bytes = sizeof(BatchFillRoi) * (size_t)B;
  void *h_meta = nullptr, *d_meta = nullptr;
  PRAD_TRY(c.get_pinned("batch_glszm_fill_meta", meta_bytes, &h_meta));
  PRAD_TRY(c.get("batch_glszm_fill_meta", meta_bytes, &d_meta));
  BatchFillRoi *rois = (BatchFillRoi *)h_meta;
  for (int b = 0; b < B; b++) {
    rois[b].zones = 2 * off[b];
    rois[b].out = out_offsets[b];
    rois[b].sizes = compact ? sizes_offsets[b] : 0;
    rois[b].nzones = summary_host[3 * b];
    rois[b].max_region = summary_host[3 * b + 1];
    rois[b].nsizes = summary_host[3 * b + 2];
    rois[b].pad = 0;
  }
  PRAD_TRY(c.begin_call(s));
  PRAD_HIP(hipMemcpyAsync(d_meta, h_meta, meta_bytes, hipMemcpyHostToDevice, s));
  int rc;
  {
    Timed t(c, "batch_glszm", s);
    hipLaunchKernelGGL(batch_glszm_fill_kernel, dim3((unsigned)B), dim3(PRAD_BZ_THREADS), 0, s, zones,
                       (const BatchFillRoi *)d_meta, Ng, compact ? 1 : 0, out, sizes_out);
    rc = check_launch("batch_glszm_fill_kernel");
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));   // (the pinned record block is reused by the next call)
  c.last_path = "batch";
  c.last_variant = "batch-glszm-lds";
  return PRAD_OK;
}
