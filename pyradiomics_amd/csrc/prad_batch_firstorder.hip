// prad_batch_firstorder.hip -- C ABI of the batched small-ROI front end (include/pyradiomics_amd.h:
// prad_batch_firstorder_max_roi, prad_batch_firstorder_plan, prad_batch_firstorder_dev, prad_batch_digitize_max_edges,
// prad_batch_digitize_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_firstorder.h"
#include "prad_batch_common.h"

#include <algorithm>

using namespace prad;

namespace {

inline int key_bytes(int dtype) { return dtype == 1 ? 8 : 4; }
inline int capacity_of(int dtype) { return PRAD_BFO_KEY_BYTES / key_bytes(dtype); }

// slots the workgroup of a box of n voxels sorts
inline int slots_of(long long n, int capacity) {
  const long long need = std::min<long long>(n, capacity);
  int P = 1;
  while (P < need) P <<= 1;
  return P;
}

// Host only: no device is touched.  *why is set (and PRAD_OK returned) when the arguments are valid but outside the domain.
int fo_batch_check(const int *sizes, int B, int dtype, long long *lds_bytes, int *inside, char *why, size_t why_len) {
  why[0] = 0;
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch firstorder: dtype %d", dtype);
  PRAD_TRY(roi_count_check("batch firstorder", sizes, B, 1));
  PRAD_TRY(roi_sizes_check("batch firstorder", sizes, B, nullptr));
  const int cap = capacity_of(dtype);
  int P = 1;
  for (int b = 0; b < B; b++) {
    const long long nvox = roi_nvox(sizes, b);
    if (!why[0] && nvox > 2147483647LL) snprintf(why, why_len, "ROI %d holds %lld voxels, above 2^31 - 1", b, nvox);
    if (inside) inside[b] = nvox <= cap ? 1 : 0;
    P = std::max(P, slots_of(nvox, cap));
  }
  *lds_bytes = PRAD_BFO_MISC_BYTES + (long long)P * key_bytes(dtype);
  return PRAD_OK;
}

}  // namespace

extern "C" int prad_batch_firstorder_max_roi(int dtype) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch firstorder: dtype %d", dtype);
  return capacity_of(dtype);
}

extern "C" int prad_batch_digitize_max_edges(void) { return PRAD_BATCH_DIGITIZE_MAX_EDGES; }

extern "C" int prad_batch_firstorder_plan(const int *sizes, int B, int dtype, long long *lds_bytes, int *inside) {
  if (!lds_bytes || !inside) return fail(PRAD_E_ARG, "batch firstorder plan: NULL output");
  char why[160];
  PRAD_TRY(fo_batch_check(sizes, B, dtype, lds_bytes, inside, why, sizeof(why)));
  if (why[0]) return fail(PRAD_E_UNSUPPORTED, "batch firstorder: %s (use the single call per ROI)", why);
  return PRAD_OK;
}

extern "C" int prad_batch_firstorder_dev(const void *image, int dtype, const uint8_t *mask, const int *sizes, const long long *off,
                                         int B, double voxelArrayShift, double *table, void *stream) {
  char why[160];
  long long lds_bytes = 0;
  PRAD_TRY(fo_batch_check(sizes, B, dtype, &lds_bytes, nullptr, why, sizeof(why)));
  if (!image || !mask || !off || !table) return fail(PRAD_E_ARG, "batch firstorder: NULL pointer");
  PRAD_TRY(roi_offsets_check("batch firstorder", off, B));
  if (why[0]) return fail(PRAD_E_UNSUPPORTED, "batch firstorder: %s (use the single call per ROI)", why);   // nothing launched
  const size_t lds = (size_t)lds_bytes;
  if (lds > 160 * 1024) return fail(PRAD_E_HIP, "batch firstorder: %zu bytes of LDS per workgroup", lds);
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  const int cap = capacity_of(dtype);

  RecordTable<BatchFoRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_fo_meta", (size_t)B));
  BatchFoRoi *rois = recs.host;
  for (int b = 0; b < B; b++) {
    const long long nvox = roi_nvox(sizes, b);
    rois[b].off = off[b];
    rois[b].n = nvox;
    rois[b].P = slots_of(nvox, cap);
    rois[b].pad = 0;
  }
  return batch_call(c, s, recs, "batch-firstorder-lds", [&]() {
    return dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      PRAD_TRY(allow_dynamic_lds(&batch_firstorder_kernel<T>, lds));
      Timed t(c, "batch_firstorder", s);
      hipLaunchKernelGGL(batch_firstorder_kernel<T>, dim3((unsigned)B), dim3(PRAD_BFO_THREADS), lds, s, (const T *)image, mask,
                         recs.dev, cap, voxelArrayShift, table);
      return check_launch("batch_firstorder_kernel");
    });
  });
}

extern "C" int prad_batch_digitize_dev(const void *image, int dtype, const uint8_t *mask, const int *sizes, const long long *off,
                                       int B, const double *edges, const long long *edge_off, int32_t *levels, long long *counts,
                                       const long long *count_off, int *top, void *stream) {
  char why[160];
  long long unused = 0;
  PRAD_TRY(fo_batch_check(sizes, B, dtype, &unused, nullptr, why, sizeof(why)));
  if (!image || !mask || !off || !edge_off || !levels || !counts || !count_off || !top)
    return fail(PRAD_E_ARG, "batch digitize: NULL pointer");
  long long most = 0, served = 0;
  for (int b = 0; b < B; b++) {
    const long long ne = edge_off[b + 1] - edge_off[b];
    if (off[b] < 0 || edge_off[b] < 0 || ne < 0) return fail(PRAD_E_ARG, "batch digitize: bad offsets of ROI %d", b);
    if (count_off[b] < 0) continue;
    served++;
    if (!why[0] && ne > PRAD_BATCH_DIGITIZE_MAX_EDGES)
      snprintf(why, sizeof(why), "ROI %d has %lld edges, above %d", b, ne, PRAD_BATCH_DIGITIZE_MAX_EDGES);
    most = std::max(most, ne);
  }
  if (most > 0 && !edges) return fail(PRAD_E_ARG, "batch digitize: NULL edges");
  if (why[0]) return fail(PRAD_E_UNSUPPORTED, "batch digitize: %s (use prad_digitize_counts_dev for that ROI)", why);   // nothing launched
  if (served == 0) return PRAD_OK;
  const size_t lds = (64 + 8 * (size_t)most + 4 * ((size_t)most + 1) + 15) & ~(size_t)15;
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  RecordTable<BatchDigRoi> table;
  PRAD_TRY(table.reserve(c, "batch_dig_meta", (size_t)B));
  BatchDigRoi *rois = table.host;
  for (int b = 0; b < B; b++) {
    const int ne = (int)(edge_off[b + 1] - edge_off[b]);
    rois[b].off = off[b];
    rois[b].n = roi_nvox(sizes, b);
    rois[b].edges = edge_off[b];
    rois[b].counts = count_off[b];
    rois[b].nedges = count_off[b] < 0 ? 0 : ne;
    int step = 1;
    while (2 * step <= rois[b].nedges) step <<= 1;
    rois[b].step = step;
  }
  return batch_call(c, s, table, "batch-digitize-lds", [&]() {
    return dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      PRAD_TRY(allow_dynamic_lds(&batch_digitize_kernel<T>, lds));
      Timed t(c, "batch_firstorder", s);
      hipLaunchKernelGGL(batch_digitize_kernel<T>, dim3((unsigned)B), dim3(PRAD_BFO_THREADS), lds, s, (const T *)image, mask,
                         table.dev, edges, levels, counts, top);
      return check_launch("batch_digitize_kernel");
    });
  });
}
