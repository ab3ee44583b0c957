// prad_batch_resample.hip -- C ABI of the batched resampling step (include/pyradiomics_amd.h: prad_batch_mask_boxes_dev,
// prad_batch_resample_dev, prad_batch_resample_max_vox); translation unit of libpyradiomics_amd.so.
#include <math.h>
#include <type_traits>

#include "kernels_batch_resample.h"
#include "prad_batch_common.h"

#include <cstring>
#include <vector>

using namespace prad;

namespace {

template <typename T>
int launch(hipStream_t s, unsigned n_bs, unsigned blocks, const void *image, const unsigned char *mask, double *coef,
           const BatchResampleRoi *rois, const int *first, const int *bs, long long total, void *out, unsigned char *out_mask) {
  if (n_bs) {
    const int horizon = (int)ceil(log(1e-10) / log(fabs(sqrt(3.0) - 2.0)));
    hipLaunchKernelGGL(batch_bspline_prefilter_kernel<T>, dim3(n_bs), dim3(PRAD_BRES_THREADS), 0, s, (const T *)image, rois, bs,
                       coef, horizon);
    PRAD_TRY(check_launch("batch_bspline_prefilter_kernel"));
  }
  hipLaunchKernelGGL(batch_resample_kernel<T>, dim3(blocks), dim3(PRAD_BRES_THREADS), 0, s, (const T *)image, mask,
                     (const double *)coef, rois, first, total, (T *)out, out_mask);
  return check_launch("batch_resample_kernel");
}

}  // namespace

// the texture route's cap: a box the resampling step takes is a box the batched matrices take
extern "C" int prad_batch_resample_max_vox(void) { return prad_batch_max_vox(); }

extern "C" int prad_batch_mask_boxes_dev(const unsigned char *mask, const int *sizes, const long long *off, int B, int *boxes,
                                         void *stream) {
  PRAD_TRY(roi_count_check("batch mask boxes", sizes, B, 0));
  if (B > 0 && (!mask || !off || !boxes)) return fail(PRAD_E_ARG, "batch mask boxes: NULL pointer");
  PRAD_TRY(roi_sizes_check("batch mask boxes", sizes, B, nullptr));
  PRAD_TRY(roi_offsets_check("batch mask boxes", off, B));
  Context &c = ctx();
  if (B == 0) {
    c.last_path = "batch";
    c.last_variant = "batch-mask-boxes";
    return PRAD_OK;
  }
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  RecordTable<MaskBoxRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_mask_boxes_meta", (size_t)B));
  for (int b = 0; b < B; b++) {
    MaskBoxRoi &r = recs.host[b];
    r.off = off[b];
    r.nz = sizes[3 * b];
    r.ny = sizes[3 * b + 1];
    r.nx = sizes[3 * b + 2];
    r.pad = 0;
  }
  int *d_boxes = nullptr;
  void *h_boxes = nullptr;
  const size_t bytes = sizeof(int) * 7 * (size_t)B;
  PRAD_TRY(c.get<int>("batch_mask_boxes_out", 7 * (size_t)B, &d_boxes));
  PRAD_TRY(c.get_pinned("batch_mask_boxes_out", bytes, &h_boxes));
  PRAD_TRY(batch_call(c, s, recs, "batch-mask-boxes", [&]() {
    {
      Timed t(c, "batch_mask_boxes", s);
      hipLaunchKernelGGL(batch_mask_boxes_kernel, dim3((unsigned)B), dim3(PRAD_BRES_THREADS), 0, s, mask, recs.dev, d_boxes);
      PRAD_TRY(check_launch("batch_mask_boxes_kernel"));
    }
    PRAD_HIP(hipMemcpyAsync(h_boxes, d_boxes, bytes, hipMemcpyDeviceToHost, s));      // the one read-back of the feature
    return (int)PRAD_OK;
  }));
  memcpy(boxes, h_boxes, bytes);            // (batch_call has waited for the stream)
  return PRAD_OK;
}

extern "C" int prad_batch_resample_dev(const void *in, int dtype, const unsigned char *mask, const int *sizes, const long long *off,
                                       int B, const double *start, const double *step, const int *newsize, const int *interp,
                                       const long long *out_off, void *out, unsigned char *out_mask, int *verdict, void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch resample: dtype %d", dtype);
  PRAD_TRY(roi_count_check("batch resample", sizes, B, 0));
  if ((mask == nullptr) != (out_mask == nullptr)) return fail(PRAD_E_ARG, "batch resample: a mask without its output (or the reverse)");
  if (B > 0 && (!in || !off || !start || !step || !newsize || !interp || !out_off || !out || !verdict))
    return fail(PRAD_E_ARG, "batch resample: NULL pointer");
  PRAD_TRY(roi_sizes_check("batch resample", sizes, B, nullptr));
  PRAD_TRY(roi_offsets_check("batch resample", off, B));
  PRAD_TRY(roi_offsets_check("batch resample (outputs)", out_off, B));
  long long end = 0;
  for (int b = 0; b < B; b++) {
    for (int d = 0; d < 3; d++) {
      if (newsize[3 * b + d] < 1) return fail(PRAD_E_ARG, "batch resample: ROI %d has newsize[%d]=%d < 1", b, d, newsize[3 * b + d]);
      if (!isfinite(start[3 * b + d]) || !isfinite(step[3 * b + d]))
        return fail(PRAD_E_ARG, "batch resample: ROI %d has a start or step along axis %d that is not finite", b, d);
    }
    if (interp[b] != 0 && interp[b] != 1 && interp[b] != 3)
      return fail(PRAD_E_ARG, "batch resample: ROI %d has interpolator %d (0 nearest, 1 linear, 3 cubic B-spline)", b, interp[b]);
    if (out_off[b] < end)
      return fail(PRAD_E_ARG, "batch resample: out_off[%d]=%lld lies before the end of ROI %d (%lld)", b, out_off[b], b - 1, end);
    end = out_off[b] + roi_nvox(newsize, b);
  }
  Context &c = ctx();
  // the native ROIs, their work items and the coefficient boxes of those the B-spline interpolates
  std::vector<int> native, bs;
  const long long max_vox = prad_batch_max_vox();
  long long total = 0, coef_len = 0;
  for (int b = 0; b < B; b++) {
    verdict[b] = roi_nvox(sizes, b) > max_vox ? 8 : 0;
    if (verdict[b] != 0) continue;
    if (interp[b] == 3) bs.push_back((int)native.size());
    native.push_back(b);
    total += roi_nvox(newsize, b);
  }
  const long long nchunks = (total + PRAD_BRES_CHUNK - 1) / PRAD_BRES_CHUNK;
  if (nchunks > 2147483647LL) return fail(PRAD_E_UNSUPPORTED, "batch resample: %lld output voxels in one call", total);
  if (native.empty()) {            // nothing for the kernels: an empty batch, or every box goes to the single route
    c.last_path = "batch";
    c.last_variant = "batch-resample";
    return PRAD_OK;
  }
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  const size_t Bn = native.size(), first_bytes = sizeof(int) * (size_t)(nchunks + 1), bs_bytes = sizeof(int) * bs.size();
  RecordTable<BatchResampleRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_resample_meta", Bn, first_bytes + bs_bytes));
  long long w = 0;
  for (size_t k = 0; k < Bn; k++) {
    const int b = native[k];
    BatchResampleRoi &r = recs.host[k];
    r.in_off = off[b];
    r.out_off = out_off[b];
    r.coef_off = coef_len;
    r.w = w;
    r.nout = roi_nvox(newsize, b);
    for (int d = 0; d < 3; d++) {
      r.start[d] = start[3 * b + d];
      r.step[d] = step[3 * b + d];
      r.in[d] = sizes[3 * b + d];
      r.out[d] = newsize[3 * b + d];
    }
    r.interp = interp[b];
    r.pad = 0;
    w += r.nout;
    if (r.interp == 3) coef_len += roi_nvox(sizes, b);
  }
  {
    // the ROI of every chunk's first item, and the last ROI behind the last chunk
    int *first = (int *)recs.host_tail();
    size_t k = 0;
    for (long long ch = 0; ch < nchunks; ch++) {
      const long long item = ch * PRAD_BRES_CHUNK;
      while (k + 1 < Bn && recs.host[k + 1].w <= item) k++;
      first[ch] = (int)k;
    }
    first[nchunks] = (int)Bn - 1;
    if (bs_bytes) memcpy((char *)recs.host_tail() + first_bytes, bs.data(), bs_bytes);
  }
  const int *d_first = (const int *)recs.dev_tail();
  const int *d_bs = (const int *)((const char *)recs.dev_tail() + first_bytes);
  double *coef = nullptr;
  if (coef_len) PRAD_TRY(c.get<double>("batch_resample_coef", (size_t)coef_len, &coef));
  return batch_call(c, s, recs, "batch-resample", [&]() {
    Timed t(c, "batch_resample", s);
    return dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch<T>(s, (unsigned)bs.size(), (unsigned)nchunks, in, mask, coef, recs.dev, d_first, d_bs, total, out, out_mask);
    });
  });
}
