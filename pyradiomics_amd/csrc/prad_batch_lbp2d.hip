// prad_batch_lbp2d.hip -- C ABI of the batched LBP2D image type (include/pyradiomics_amd.h: prad_batch_lbp2d_plan,
// prad_batch_lbp2d_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_lbp2d.h"
#include "prad_batch_common.h"
#include "prad_lbp2d_check.h"

using namespace prad;

namespace {

// the arguments both entry points share; host only
int lbp_batch_check(const char *what, const int *sizes, int B, int axis) {
  PRAD_TRY(roi_count_check(what, sizes, B, 1));
  PRAD_TRY(roi_sizes_check(what, sizes, B, nullptr));
  if (axis < 0 || axis > 2) return fail(PRAD_E_ARG, "%s: axis=%d outside 0 .. 2", what, axis);
  return PRAD_OK;
}

template <typename T>
int launch(Context &c, hipStream_t s, const Lbp2dPlan &p, const LbpGeom &g, const LbpTable &tab, const void *in, double *out,
           const BatchLbpRoi *rois, const BatchLbpItem *items) {
  Timed t(c, "batch_lbp2d", s);
  hipLaunchKernelGGL(batch_lbp2d_kernel<T>, dim3((unsigned)p.groups), dim3(kLbpThreads), (size_t)p.lds, s, (const T *)in, out, rois,
                     items, g, tab);
  return check_launch("batch_lbp2d_kernel");
}

}  // namespace

extern "C" int prad_batch_lbp2d_plan(const int *sizes, int B, int axis, int halo, int *tile, long long *n_items, int *items,
                                     long long *lds_bytes, int *verdict) {
  PRAD_TRY(lbp_batch_check("batch lbp2d plan", sizes, B, axis));
  if (!tile || !n_items || !lds_bytes || !verdict) return fail(PRAD_E_ARG, "batch lbp2d plan: NULL output");
  const Lbp2dPlan p = batch_lbp2d_plan(sizes, B, axis, halo, (BatchLbpItem *)items);
  for (int d = 0; d < 3; d++) tile[d] = p.tile[d];
  *n_items = p.groups;
  *lds_bytes = p.lds;
  *verdict = p.verdict;
  return PRAD_OK;
}

extern "C" int prad_batch_lbp2d_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, int axis,
                                    const double *rp, const double *cp, int P, int halo, int method, double *out, void *stream) {
  PRAD_TRY(lbp_batch_check("batch lbp2d", sizes, B, axis));
  if (!in || !off || !out) return fail(PRAD_E_ARG, "batch lbp2d: NULL pointer");
  if (in == (const void *)out) return fail(PRAD_E_ARG, "batch lbp2d: the images cannot be filtered in place");
  PRAD_TRY(roi_offsets_check("batch lbp2d", off, B));
  // the boxes follow one another: the image of ROI b must not reach into ROI b + 1
  long long end = 0;
  for (int b = 0; b < B; b++) {
    if (off[b] < end) return fail(PRAD_E_ARG, "batch lbp2d: off[%d]=%lld lies before the end of ROI %d (%lld)", b, off[b], b - 1, end);
    end = off[b] + roi_nvox(sizes, b);
  }
  LbpTable tab;
  PRAD_TRY(lbp_args_check("batch lbp2d", dtype, 1, rp, cp, P, halo, method, &tab));
  Lbp2dPlan p = batch_lbp2d_plan(sizes, B, axis, halo, nullptr);
  if (p.verdict != kLbpNative)
    return fail(PRAD_E_UNSUPPORTED, "batch lbp2d: %s", p.verdict == kLbpGrid ? "more workgroups than one launch holds" : "no tile fits the LDS budget");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  RecordTable<BatchLbpRoi> recs;
  PRAD_TRY(recs.reserve(c, "batch_lbp2d_meta", (size_t)B, sizeof(BatchLbpItem) * (size_t)p.groups));
  p = batch_lbp2d_plan(sizes, B, axis, halo, (BatchLbpItem *)recs.host_tail());
  for (int b = 0; b < B; b++) {
    BatchLbpRoi &r = recs.host[b];
    r.off = off[b];
    r.nz = sizes[3 * b];
    r.ny = sizes[3 * b + 1];
    r.nx = sizes[3 * b + 2];
    r.pad = 0;
  }
  const BatchLbpItem *items = (const BatchLbpItem *)recs.dev_tail();
  const LbpGeom g = lbp_geom(p, axis, halo, P, method);
  return batch_call(c, s, recs, "batch-lbp2d", [&]() {
    return dispatch_image_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      return launch<T>(c, s, p, g, tab, in, out, recs.dev, items);
    });
  });
}
