// prad_resegment.hip -- C ABI of the resegmentation of one volume (include/pyradiomics_amd.h: prad_resegment_dev); translation
// unit of libpyradiomics_amd.so.
#include <math.h>

#include "kernels_resegment.h"
#include "prad_batch_common.h"

#include <algorithm>
#include <cstring>

using namespace prad;

namespace {

template <typename T, typename L>
int launch(hipStream_t s, const void *image, const void *lab, const ResegGeo &g, int label, const ResegRange &r, void *partial,
           double *ssd, void *out, ResegSummary *sum) {
  const dim3 grid((unsigned)g.groups), block(PRAD_RESEG_THREADS);
  ResegStats<T> *part = (ResegStats<T> *)partial;
  if (r.mode == PRAD_RESEG_ABSOLUTE) {
    hipLaunchKernelGGL(reseg_init_kernel, dim3(1), dim3(1), 0, s, sum, g);
    PRAD_TRY(check_launch("reseg_init_kernel"));
  } else {
    hipLaunchKernelGGL((reseg_stats_kernel<T, L>), grid, block, 0, s, (const T *)image, (const L *)lab, g, label, part, sum);
    PRAD_TRY(check_launch("reseg_stats_kernel"));
  }
  if (r.mode == PRAD_RESEG_SIGMA) {
    hipLaunchKernelGGL((reseg_ssd_kernel<T, L>), grid, block, 0, s, (const T *)image, (const L *)lab, g, label,
                       (const ResegStats<T> *)part, ssd);
    PRAD_TRY(check_launch("reseg_ssd_kernel"));
  }
  hipLaunchKernelGGL((reseg_mask_kernel<T, L>), grid, block, 0, s, (const T *)image, (const L *)lab, g, label, r,
                     (const ResegStats<T> *)part, (const double *)ssd, (L *)out, sum);
  return check_launch("reseg_mask_kernel");
}

template <typename T>
int launch_label(int label_dtype, hipStream_t s, const void *image, const void *lab, const ResegGeo &g, int label,
                 const ResegRange &r, void *partial, double *ssd, void *out, ResegSummary *sum) {
  switch (label_dtype) {
    case 2: return launch<T, int>(s, image, lab, g, label, r, partial, ssd, out, sum);
    case 3: return launch<T, short>(s, image, lab, g, label, r, partial, ssd, out, sum);
    default: return launch<T, unsigned char>(s, image, lab, g, label, r, partial, ssd, out, sum);
  }
}

}  // namespace

extern "C" int prad_resegment_dev(const void *image, int dtype, const void *labelmap, int label_dtype, const int *size, int Nd,
                                  int label, int mode, const double *range, int nrange, void *out_mask, long long *counts,
                                  int *box, double *thr, void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "resegment: dtype %d (0 float32, 1 float64, 2 int32, 3 int16)", dtype);
  if (label_dtype < 2 || label_dtype > 4)
    return fail(PRAD_E_ARG, "resegment: label dtype code %d (2 int32, 3 int16, 4 uint8)", label_dtype);
  ResegRange r;
  PRAD_TRY(resegment_range_check("resegment", mode, range, nrange, &r));
  if (!image || !labelmap || !size || !out_mask || !counts || !box || !thr) return fail(PRAD_E_ARG, "resegment: NULL pointer");
  if (Nd < 1 || Nd > 3) return fail(PRAD_E_ARG, "resegment: Nd=%d (1, 2 or 3)", Nd);
  Geo geo;
  PRAD_TRY(make_geo(size, Nd, &geo));
  if (mode == PRAD_RESEG_SIGMA && dtype == 0)      // np.mean / np.std of a float32 array accumulate in float32: the host's job
    return fail(PRAD_E_UNSUPPORTED, "resegment: sigma mode on a float32 image is not served on the device");
  ResegGeo g;
  g.n = geo.n;
  g.nx = size[Nd - 1];
  g.ny = Nd >= 2 ? size[Nd - 2] : 1;
  g.nz = Nd == 3 ? size[0] : 1;
  // the grid follows from the voxel count alone, so the order of every sum does too
  const long long per_group = (long long)PRAD_RESEG_THREADS * PRAD_RESEG_PER_LANE;
  g.groups = (int)std::max<long long>(1, std::min<long long>((g.n + per_group - 1) / per_group, PRAD_RESEG_MAX_GROUPS));

  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  void *partial = nullptr, *h_sum = nullptr;
  double *ssd = nullptr;
  ResegSummary *d_sum = nullptr;
  PRAD_TRY(c.get("resegment_partial", sizeof(ResegStats<double>) * (size_t)PRAD_RESEG_MAX_GROUPS, &partial));
  PRAD_TRY(c.get<double>("resegment_ssd", (size_t)PRAD_RESEG_MAX_GROUPS, &ssd));
  PRAD_TRY(c.get<ResegSummary>("resegment_summary", 1, &d_sum));
  PRAD_TRY(c.get_pinned("resegment_summary", sizeof(ResegSummary), &h_sum));
  PRAD_TRY(c.begin_call(s));
  int rc;
  {
    Timed t(c, "resegment", s);
    rc = dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch_label<T>(label_dtype, s, image, labelmap, g, label, r, partial, ssd, out_mask, d_sum);
    });
  }
  PRAD_TRY(c.end_call(s));
  if (rc != PRAD_OK) return rc;
  PRAD_HIP(hipMemcpyAsync(h_sum, d_sum, sizeof(ResegSummary), hipMemcpyDeviceToHost, s));      // the one read-back
  PRAD_HIP(hipStreamSynchronize(s));
  c.last_path = "resegment";
  c.last_variant = mode == PRAD_RESEG_ABSOLUTE ? "resegment-absolute" : (mode == PRAD_RESEG_RELATIVE ? "resegment-relative" : "resegment-sigma");
  const ResegSummary *h = (const ResegSummary *)h_sum;
  if (h->nonfinite)
    return fail(PRAD_E_UNSUPPORTED, "resegment: a non-finite value inside the ROI (the output mask is not valid)");
  counts[0] = (long long)h->before;
  counts[1] = (long long)h->after;
  for (int d = 0; d < 3; d++) {
    box[d] = h->lo[d];
    box[3 + d] = h->hi[d];
  }
  thr[0] = h->thr[0];
  thr[1] = h->thr[1];
  return PRAD_OK;
}
