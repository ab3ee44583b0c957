// prad_batch_resegment.hip -- C ABI of the batched resegmentation (include/pyradiomics_amd.h: prad_batch_resegment_dev);
// translation unit of libpyradiomics_amd.so.
#include <math.h>

#include "kernels_batch_resegment.h"
#include "prad_batch_common.h"

#include <cstring>

using namespace prad;

extern "C" int prad_batch_resegment_dev(const void *image, int dtype, const unsigned char *mask, const int *sizes,
                                        const long long *off, int B, int mode, const double *range, int nrange,
                                        unsigned char *out_mask, int *boxes, double *thr, int *verdict, void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch resegment: dtype %d", dtype);
  ResegRange r;
  PRAD_TRY(resegment_range_check("batch resegment", mode, range, nrange, &r));
  PRAD_TRY(roi_count_check("batch resegment", sizes, B, 0));
  if (B > 0 && (!image || !mask || !off || !out_mask || !boxes || !thr || !verdict))
    return fail(PRAD_E_ARG, "batch resegment: NULL pointer");
  PRAD_TRY(roi_sizes_check("batch resegment", sizes, B, nullptr));
  PRAD_TRY(roi_offsets_check("batch resegment", off, B));
  Context &c = ctx();
  if (B == 0) {            // an empty batch: nothing for the kernel
    c.last_path = "batch";
    c.last_variant = "batch-resegment";
    return PRAD_OK;
  }
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  const long long cap = prad_batch_max_vox();
  const bool sigma32 = mode == PRAD_RESEG_SIGMA && dtype == 0;      // numpy's float32 mean and sigma: the host's job
  RecordTable<BatchResegRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_resegment_meta", (size_t)B));
  for (int b = 0; b < B; b++) {
    BatchResegRoi &roi = recs.host[b];
    roi.off = off[b];
    roi.nz = sizes[3 * b];
    roi.ny = sizes[3 * b + 1];
    roi.nx = sizes[3 * b + 2];
    roi.served = !sigma32 && roi_nvox(sizes, b) <= cap;
  }
  BatchResegRow *d_rows = nullptr;
  void *h_rows = nullptr;
  const size_t bytes = sizeof(BatchResegRow) * (size_t)B;
  PRAD_TRY(c.get<BatchResegRow>("batch_resegment_rows", (size_t)B, &d_rows));
  PRAD_TRY(c.get_pinned("batch_resegment_rows", bytes, &h_rows));
  PRAD_TRY(batch_call(c, s, recs, "batch-resegment", [&]() {
    {
      Timed t(c, "batch_resegment", s);
      PRAD_TRY(dispatch_image_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(batch_resegment_kernel<T>, dim3((unsigned)B), dim3(PRAD_RESEG_THREADS), 0, s, (const T *)image, mask,
                           recs.dev, r, out_mask, d_rows);
        return check_launch("batch_resegment_kernel");
      }));
    }
    PRAD_HIP(hipMemcpyAsync(h_rows, d_rows, bytes, hipMemcpyDeviceToHost, s));      // the one read-back
    return (int)PRAD_OK;
  }));
  const BatchResegRow *rows = (const BatchResegRow *)h_rows;      // (batch_call has waited for the stream)
  for (int b = 0; b < B; b++) {
    memcpy(boxes + 7 * (size_t)b, rows[b].box, sizeof(int) * 7);
    thr[2 * (size_t)b] = rows[b].thr[0];
    thr[2 * (size_t)b + 1] = rows[b].thr[1];
    verdict[b] = rows[b].verdict;
  }
  return PRAD_OK;
}
