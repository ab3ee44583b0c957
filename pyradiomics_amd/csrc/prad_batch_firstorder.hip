// prad_batch_firstorder.hip -- C ABI of the batched small-ROI front end (include/pyradiomics_amd.h:
// prad_batch_firstorder_max_roi, prad_batch_firstorder_plan, prad_batch_firstorder_dev, prad_batch_digitize_max_edges,
// prad_batch_digitize_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_firstorder.h"

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
  if (B < 1 || !sizes) return fail(PRAD_E_ARG, "batch firstorder: B=%d, sizes=%p", B, (const void *)sizes);
  const int cap = capacity_of(dtype);
  int P = 1;
  for (int b = 0; b < B; b++) {
    const int *sz = sizes + 3 * b;
    for (int d = 0; d < 3; d++)
      if (sz[d] < 1) return fail(PRAD_E_ARG, "batch firstorder: ROI %d has size[%d]=%d < 1", b, d, sz[d]);
    const long long nvox = (long long)sz[0] * sz[1] * sz[2];
    if (!why[0] && nvox > 2147483647LL) snprintf(why, why_len, "ROI %d holds %lld voxels, above 2^31 - 1", b, nvox);
    if (inside) inside[b] = nvox <= cap ? 1 : 0;
    P = std::max(P, slots_of(nvox, cap));
  }
  *lds_bytes = PRAD_BFO_MISC_BYTES + (long long)P * key_bytes(dtype);
  return PRAD_OK;
}

template <typename T>
int launch_firstorder(Context &c, hipStream_t s, const void *image, const uint8_t *mask, const BatchFoRoi *rois, int B, int cap,
                      size_t lds, double shift, double *table) {
  if (lds > 64 * 1024)
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&batch_firstorder_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  Timed t(c, "batch_firstorder", s);
  hipLaunchKernelGGL(batch_firstorder_kernel<T>, dim3((unsigned)B), dim3(PRAD_BFO_THREADS), lds, s, (const T *)image, mask, rois, cap,
                     shift, table);
  return check_launch("batch_firstorder_kernel");
}

template <typename T>
int launch_digitize(Context &c, hipStream_t s, const void *image, const uint8_t *mask, const BatchDigRoi *rois, int B, size_t lds,
                    const double *edges, int *levels, long long *counts, int *top) {
  if (lds > 64 * 1024)
    PRAD_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&batch_digitize_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  Timed t(c, "batch_firstorder", s);
  hipLaunchKernelGGL(batch_digitize_kernel<T>, dim3((unsigned)B), dim3(PRAD_BFO_THREADS), lds, s, (const T *)image, mask, rois, edges,
                     levels, counts, top);
  return check_launch("batch_digitize_kernel");
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
  for (int b = 0; b < B; b++)
    if (off[b] < 0) return fail(PRAD_E_ARG, "batch firstorder: off[%d]=%lld < 0", b, off[b]);
  if (why[0]) return fail(PRAD_E_UNSUPPORTED, "batch firstorder: %s (use the single call per ROI)", why);   // nothing launched
  const size_t lds = (size_t)lds_bytes;
  if (lds > 160 * 1024) return fail(PRAD_E_HIP, "batch firstorder: %zu bytes of LDS per workgroup", lds);
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  const int cap = capacity_of(dtype);

  const size_t meta_bytes = sizeof(BatchFoRoi) * (size_t)B;
  void *h_meta = nullptr, *d_meta = nullptr;
  PRAD_TRY(c.get_pinned("batch_fo_meta", meta_bytes, &h_meta));
  PRAD_TRY(c.get("batch_fo_meta", meta_bytes, &d_meta));
  BatchFoRoi *rois = (BatchFoRoi *)h_meta;
  for (int b = 0; b < B; b++) {
    const long long nvox = (long long)sizes[3 * b] * sizes[3 * b + 1] * sizes[3 * b + 2];
    rois[b].off = off[b];
    rois[b].n = nvox;
    rois[b].P = slots_of(nvox, cap);
    rois[b].pad = 0;
  }
  PRAD_TRY(c.begin_call(s));
  PRAD_HIP(hipMemcpyAsync(d_meta, h_meta, meta_bytes, hipMemcpyHostToDevice, s));
  int rc;
  const BatchFoRoi *dr = (const BatchFoRoi *)d_meta;
  switch (dtype) {
    case 0: rc = launch_firstorder<float>(c, s, image, mask, dr, B, cap, lds, voxelArrayShift, table); break;
    case 1: rc = launch_firstorder<double>(c, s, image, mask, dr, B, cap, lds, voxelArrayShift, table); break;
    case 2: rc = launch_firstorder<int>(c, s, image, mask, dr, B, cap, lds, voxelArrayShift, table); break;
    default: rc = launch_firstorder<short>(c, s, image, mask, dr, B, cap, lds, voxelArrayShift, table); break;
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));   // (the pinned record block is reused by the next call)
  c.last_path = "batch";
  c.last_variant = "batch-firstorder-lds";
  return PRAD_OK;
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

  const size_t meta_bytes = sizeof(BatchDigRoi) * (size_t)B;
  void *h_meta = nullptr, *d_meta = nullptr;
  PRAD_TRY(c.get_pinned("batch_dig_meta", meta_bytes, &h_meta));
  PRAD_TRY(c.get("batch_dig_meta", meta_bytes, &d_meta));
  BatchDigRoi *rois = (BatchDigRoi *)h_meta;
  for (int b = 0; b < B; b++) {
    const int ne = (int)(edge_off[b + 1] - edge_off[b]);
    rois[b].off = off[b];
    rois[b].n = (long long)sizes[3 * b] * sizes[3 * b + 1] * sizes[3 * b + 2];
    rois[b].edges = edge_off[b];
    rois[b].counts = count_off[b];
    rois[b].nedges = count_off[b] < 0 ? 0 : ne;
    int step = 1;
    while (2 * step <= rois[b].nedges) step <<= 1;
    rois[b].step = step;
  }
  PRAD_TRY(c.begin_call(s));
  PRAD_HIP(hipMemcpyAsync(d_meta, h_meta, meta_bytes, hipMemcpyHostToDevice, s));
  int rc;
  const BatchDigRoi *dr = (const BatchDigRoi *)d_meta;
  switch (dtype) {
    case 0: rc = launch_digitize<float>(c, s, image, mask, dr, B, lds, edges, levels, counts, top); break;
    case 1: rc = launch_digitize<double>(c, s, image, mask, dr, B, lds, edges, levels, counts, top); break;
    case 2: rc = launch_digitize<int>(c, s, image, mask, dr, B, lds, edges, levels, counts, top); break;
    default: rc = launch_digitize<short>(c, s, image, mask, dr, B, lds, edges, levels, counts, top); break;
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipStreamSynchronize(s));   // (the pinned record block is reused by the next call)
  c.last_path = "batch";
  c.last_variant = "batch-digitize-lds";
  return PRAD_OK;
}
