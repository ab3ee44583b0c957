// prad_batch_swt.hip -- C ABI of the batched wavelet transform (include/pyradiomics_amd.h: prad_batch_swt_plan,
// prad_batch_swt_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_swt.h"
#include "prad_batch_common.h"

#include <vector>

using namespace prad;

namespace {

// the arguments both entry points share; host only.  PRAD_E_UNSUPPORTED (nothing planned) for a filter length the kernel is
// not instantiated for.
int swt_batch_check(const char *what, const int *sizes, int B, int flen) {
  if (flen < 2 || flen > PRAD_MAX_TAPS) return fail(PRAD_E_ARG, "%s: filter length flen=%d outside [2,%d]", what, flen, PRAD_MAX_TAPS);
  PRAD_TRY(roi_count_check(what, sizes, B, 1));
  PRAD_TRY(roi_sizes_check(what, sizes, B, nullptr));
  return PRAD_OK;
}

int swt_flen_check(const char *what, int flen) {
  if (!bswt_flen_native(flen))
    return fail(PRAD_E_UNSUPPORTED, "%s: filter length flen=%d (the kernel is built for 2, 4 and 6 taps; use the single call per ROI)",
                what, flen);
  return PRAD_OK;
}

template <int F, typename T>
int launch(Context &c, hipStream_t s, unsigned blocks, const void *in, const BatchSwtRoi *rois, const BatchSwtItem *items,
           const BatchSwtTaps &taps, double *out, long long band_stride) {
  const size_t lds = sizeof(double) * PRAD_BSWT_LDS_DOUBLES(F);
  Timed t(c, "batch_swt", s);
  hipLaunchKernelGGL((batch_swt_kernel<F, T>), dim3(blocks), dim3(PRAD_BSWT_THREADS), lds, s, (const T *)in, rois, items, taps, out,
                     band_stride);
  return check_launch("batch_swt_kernel");
}

}  // namespace

extern "C" int prad_batch_swt_plan(const int *sizes, int B, int flen, int *verdict, long long *n_items, int *items) {
  PRAD_TRY(swt_batch_check("batch swt plan", sizes, B, flen));
  if (!verdict || !n_items) return fail(PRAD_E_ARG, "batch swt plan: NULL output");
  PRAD_TRY(swt_flen_check("batch swt plan", flen));
  batch_swt_plan(sizes, B, flen, verdict, n_items, (BatchSwtItem *)items, nullptr);
  return PRAD_OK;
}

extern "C" int prad_batch_swt_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, const double *dec_lo,
                                  const double *dec_hi, int flen, double *out, long long band_stride, int *verdict, void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch swt: dtype %d", dtype);
  PRAD_TRY(swt_batch_check("batch swt", sizes, B, flen));
  if (!in || !off || !dec_lo || !dec_hi || !out || !verdict) return fail(PRAD_E_ARG, "batch swt: NULL pointer");
  PRAD_TRY(roi_offsets_check("batch swt", off, B));
  // the boxes follow one another: band k of ROI b must not reach into ROI b + 1, nor the last box into band k + 1
  long long end = 0;
  for (int b = 0; b < B; b++) {
    if (off[b] < end) return fail(PRAD_E_ARG, "batch swt: off[%d]=%lld lies before the end of ROI %d (%lld)", b, off[b], b - 1, end);
    end = off[b] + roi_nvox(sizes, b);
  }
  if (band_stride < end) return fail(PRAD_E_ARG, "batch swt: band_stride=%lld, the boxes end at %lld", band_stride, end);
  PRAD_TRY(swt_flen_check("batch swt", flen));      // nothing launched
  long long n_items = 0;
  batch_swt_plan(sizes, B, flen, verdict, &n_items, nullptr, nullptr);
  if (n_items > 2147483647LL) return fail(PRAD_E_UNSUPPORTED, "batch swt: %lld workgroups in one call", n_items);
  if (n_items == 0) return PRAD_OK;                 // every ROI takes the single route
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  RecordTable<BatchSwtRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_swt_meta", (size_t)B, sizeof(BatchSwtItem) * (size_t)n_items));
  std::vector<int> ltx((size_t)B, 5);
  batch_swt_plan(sizes, B, flen, verdict, &n_items, (BatchSwtItem *)recs.host_tail(), ltx.data());
  for (int b = 0; b < B; b++) {
    BatchSwtRoi &r = recs.host[b];
    r.off = off[b];
    r.nz = sizes[3 * b];
    r.ny = sizes[3 * b + 1];
    r.nx = sizes[3 * b + 2];
    r.ltx = ltx[(size_t)b];
    r.pad[0] = r.pad[1] = 0;
  }
  BatchSwtTaps taps;
  for (int k = 0; k < PRAD_BSWT_MAX_F; k++) {
    taps.lo[k] = k < flen ? dec_lo[k] : 0.0;
    taps.hi[k] = k < flen ? dec_hi[k] : 0.0;
  }
  const BatchSwtItem *items = (const BatchSwtItem *)recs.dev_tail();
  const unsigned blocks = (unsigned)n_items;
  return batch_call(c, s, recs, "batch-swt-fused", [&]() {
    return dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      if (flen == 6) return launch<6, T>(c, s, blocks, in, recs.dev, items, taps, out, band_stride);
      if (flen == 4) return launch<4, T>(c, s, blocks, in, recs.dev, items, taps, out, band_stride);
      return launch<2, T>(c, s, blocks, in, recs.dev, items, taps, out, band_stride);
    });
  });
}
