// prad_batch_intensity.hip -- C ABI of the batched intensity transforms and Gradient magnitude (include/pyradiomics_amd.h:
// prad_batch_intensity_plan, prad_batch_intensity_dev); translation unit of libpyradiomics_amd.so.
#include <math.h>

#include "kernels_batch_intensity.h"
#include "prad_batch_common.h"

#include <cstring>

using namespace prad;

namespace {

// the arguments both entry points share; host only.  *n_items = the workgroups of launch 2.
int intensity_batch_check(const char *what, const int *sizes, int B, int types, long long *n_items) {
  PRAD_TRY(roi_count_check(what, sizes, B, 0));
  if (types < 1 || types > PRAD_BINT_ALL)
    return fail(PRAD_E_ARG, "%s: types=%d (bits: 1 square, 2 squareroot, 4 logarithm, 8 exponential, 16 gradient)", what, types);
  PRAD_TRY(roi_sizes_check(what, sizes, B, nullptr));
  batch_intensity_plan(sizes, B, n_items, nullptr);
  if (*n_items > PRAD_BINT_MAX_GROUPS || B > PRAD_BINT_MAX_GROUPS)
    return fail(PRAD_E_UNSUPPORTED, "%s: %d ROIs and %lld workgroups in one call (at most %lld each)", what, B, *n_items,
                PRAD_BINT_MAX_GROUPS);
  return PRAD_OK;
}

template <typename T>
int launch(Context &c, hipStream_t s, unsigned B, unsigned blocks, int types, const void *in, const BatchIntRoi *rois,
           const BatchIntItem *items, BatchIntConsts *consts, int *d_verdict, double *out64, long long row_stride, float *out_grad) {
  Timed t(c, "batch_intensity", s);
  if (types & PRAD_BINT_POINTWISE) {
    hipLaunchKernelGGL(batch_intensity_consts_kernel<T>, dim3(B), dim3(PRAD_BINT_THREADS), 0, s, (const T *)in, rois, consts,
                       d_verdict);
    PRAD_TRY(check_launch("batch_intensity_consts_kernel"));
  }
  hipLaunchKernelGGL(batch_intensity_kernel<T>, dim3(blocks), dim3(PRAD_BINT_THREADS), 0, s, (const T *)in, rois, items,
                     (const BatchIntConsts *)consts, d_verdict, types, out64, row_stride, out_grad);
  return check_launch("batch_intensity_kernel");
}

}  // namespace

extern "C" int prad_batch_intensity_plan(const int *sizes, int B, int types, long long *n_items, long long *items, long long *grid) {
  long long n = 0;
  PRAD_TRY(intensity_batch_check("batch intensity plan", sizes, B, types, &n));
  if (!n_items || !grid) return fail(PRAD_E_ARG, "batch intensity plan: NULL output");
  batch_intensity_plan(sizes, B, n_items, (BatchIntItem *)items);
  grid[0] = (types & PRAD_BINT_POINTWISE) && B > 0 ? B : 0;
  grid[1] = n;
  return PRAD_OK;
}

extern "C" int prad_batch_intensity_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, int types,
                                        const double *spacing, int gradientUseSpacing, double *out64, long long row_stride,
                                        float *out_grad, int *verdict, void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch intensity: dtype %d", dtype);
  long long n_items = 0;
  PRAD_TRY(intensity_batch_check("batch intensity", sizes, B, types, &n_items));
  const bool pointwise = (types & PRAD_BINT_POINTWISE) != 0, gradient = (types & PRAD_BINT_GRADIENT) != 0;
  if (B > 0 && (!in || !off || !verdict || (pointwise && !out64) || (gradient && !out_grad)))
    return fail(PRAD_E_ARG, "batch intensity: NULL pointer");
  PRAD_TRY(roi_offsets_check("batch intensity", off, B));
  // the boxes follow one another: the image of ROI b must not reach into ROI b + 1, nor the last box into the next row
  long long end = 0;
  for (int b = 0; b < B; b++) {
    if (off[b] < end)
      return fail(PRAD_E_ARG, "batch intensity: off[%d]=%lld lies before the end of ROI %d (%lld)", b, off[b], b - 1, end);
    end = off[b] + roi_nvox(sizes, b);
  }
  if (pointwise && row_stride < end) return fail(PRAD_E_ARG, "batch intensity: row_stride=%lld, the boxes end at %lld", row_stride, end);
  const bool scaled = gradient && gradientUseSpacing && spacing;
  if (scaled)
    for (int b = 0; b < B; b++)
      for (int d = 0; d < 3; d++)
        if (!(spacing[3 * b + d] > 0.0) || !isfinite(spacing[3 * b + d]))
          return fail(PRAD_E_ARG, "batch intensity: ROI %d has spacing[%d]=%g, must be > 0 and finite", b, d, spacing[3 * b + d]);
  Context &c = ctx();
  if (B == 0) {            // an empty batch: nothing for the kernels
    c.last_path = "batch";
    c.last_variant = "batch-intensity";
    return PRAD_OK;
  }
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  // one upload: the records, the items of launch 2 and B zero verdicts (launch 1 overwrites them; Gradient alone raises them)
  const size_t items_bytes = sizeof(BatchIntItem) * (size_t)n_items, verdict_bytes = sizeof(int) * (size_t)B;
  RecordTable<BatchIntRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_intensity_meta", (size_t)B, items_bytes + verdict_bytes));
  batch_intensity_plan(sizes, B, &n_items, (BatchIntItem *)recs.host_tail());
  memset((char *)recs.host_tail() + items_bytes, 0, verdict_bytes);
  long long w = 0;
  for (int b = 0; b < B; b++) {
    BatchIntRoi &r = recs.host[b];
    r.w = w;
    r.n = roi_nvox(sizes, b);
    r.off = off[b];
    r.nz = sizes[3 * b];
    r.ny = sizes[3 * b + 1];
    r.nx = sizes[3 * b + 2];
    r.pad = 0;
    for (int d = 0; d < 3; d++) r.inv[d] = scaled ? 1.0 / spacing[3 * b + d] : 1.0;
    w += r.n;
  }
  const BatchIntItem *d_items = (const BatchIntItem *)recs.dev_tail();
  int *d_verdict = (int *)((char *)const_cast<void *>(recs.dev_tail()) + items_bytes);
  BatchIntConsts *consts = nullptr;
  if (pointwise) PRAD_TRY(c.get<BatchIntConsts>("batch_intensity_consts", (size_t)B, &consts));
  void *h_verdict = nullptr;
  PRAD_TRY(c.get_pinned("batch_intensity_verdict", verdict_bytes, &h_verdict));
  PRAD_TRY(batch_call(c, s, recs, gradient && !pointwise ? "batch-gradient" : "batch-intensity", [&]() {
    PRAD_TRY(dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch<T>(c, s, (unsigned)B, (unsigned)n_items, types, in, recs.dev, d_items, consts, d_verdict, out64, row_stride,
                       out_grad);
    }));
    PRAD_HIP(hipMemcpyAsync(h_verdict, d_verdict, verdict_bytes, hipMemcpyDeviceToHost, s));      // the one read-back
    return (int)PRAD_OK;
  }));
  memcpy(verdict, h_verdict, verdict_bytes);      // (batch_call has waited for the stream)
  return PRAD_OK;
}
