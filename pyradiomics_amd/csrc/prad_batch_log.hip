// prad_batch_log.hip -- C ABI of the batched Laplacian of Gaussian (include/pyradiomics_amd.h: prad_batch_log_plan,
// prad_batch_log_dev); translation unit of libpyradiomics_amd.so.
#include "kernels_batch_log.h"
#include "prad_batch_common.h"

#include <cstring>
#include <map>
#include <tuple>
#include <vector>

using namespace prad;

namespace {

// the arguments both entry points share; host only
int log_batch_check(const char *what, const int *sizes, int B, const double *spacing, const double *sigmas, int S) {
  PRAD_TRY(roi_count_check(what, sizes, B, 1));
  if (!spacing || !sigmas) return fail(PRAD_E_ARG, "%s: NULL pointer", what);
  if (S < 1 || S > PRAD_BLOG_MAXSIG) return fail(PRAD_E_ARG, "%s: S=%d sigmas per call outside [1, %d]", what, S, PRAD_BLOG_MAXSIG);
  PRAD_TRY(roi_sizes_check(what, sizes, B, nullptr));
  for (int s = 0; s < S; s++)
    if (!(sigmas[s] > 0.0)) return fail(PRAD_E_ARG, "%s: sigma[%d]=%g must be > 0", what, s, sigmas[s]);
  for (int b = 0; b < B; b++)
    for (int d = 0; d < 3; d++)
      if (!(spacing[3 * b + d] > 0.0))
        return fail(PRAD_E_ARG, "%s: ROI %d has spacing[%d]=%g, must be > 0", what, b, d, spacing[3 * b + d]);
  return PRAD_OK;
}

template <typename T, int MAXT>
int launch(Context &c, hipStream_t s, unsigned blocks, size_t lds, const void *in, const BatchLogRoi *rois,
           const BatchLogItem *items, const RGaussCoef *coefs, void *out, long long row_stride) {
  PRAD_TRY(allow_dynamic_lds(batch_log_kernel<T, MAXT>, lds));
  hipLaunchKernelGGL((batch_log_kernel<T, MAXT>), dim3(blocks), dim3(MAXT), lds, s, (const T *)in, rois, items, coefs, out,
                     row_stride);
  return check_launch("batch_log_kernel");
}

}  // namespace

extern "C" int prad_batch_log_plan(const int *sizes, int B, const double *spacing, const double *sigmas, int S, int *verdict,
                                   int *lds_class, long long *n_items) {
  PRAD_TRY(log_batch_check("batch log plan", sizes, B, spacing, sigmas, S));
  if (!verdict || !lds_class || !n_items) return fail(PRAD_E_ARG, "batch log plan: NULL output");
  batch_log_plan(sizes, B, spacing, sigmas, S, verdict, lds_class, n_items);
  return PRAD_OK;
}

extern "C" int prad_batch_log_dev(const void *in, int dtype, const int *sizes, const long long *off, int B, const double *spacing,
                                  const double *sigmas, int S, int normalize, void *out, long long row_stride, int *verdict,
                                  void *stream) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "batch log: dtype %d", dtype);
  PRAD_TRY(log_batch_check("batch log", sizes, B, spacing, sigmas, S));
  if (!in || !off || !out || !verdict) return fail(PRAD_E_ARG, "batch log: NULL pointer");
  PRAD_TRY(roi_offsets_check("batch log", off, B));
  // the boxes follow one another: the image of ROI b must not reach into ROI b + 1, nor the last box into the next row
  long long end = 0;
  for (int b = 0; b < B; b++) {
    if (off[b] < end) return fail(PRAD_E_ARG, "batch log: off[%d]=%lld lies before the end of ROI %d (%lld)", b, off[b], b - 1, end);
    end = off[b] + roi_nvox(sizes, b);
  }
  if (row_stride < end) return fail(PRAD_E_ARG, "batch log: row_stride=%lld, the boxes end at %lld", row_stride, end);
  std::vector<int> cls((size_t)B);
  long long n_items = 0;
  batch_log_plan(sizes, B, spacing, sigmas, S, verdict, cls.data(), &n_items);
  if (n_items > 2147483647LL) return fail(PRAD_E_UNSUPPORTED, "batch log: %lld workgroups in one call", n_items);
  if (n_items == 0) return PRAD_OK;                 // nothing for the kernel: the single route, or no image at all
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;

  // one RGaussCoef per distinct (sigma, spacing of an axis, order), in the order the items meet them
  std::map<std::tuple<double, double, int>, int> seen;
  std::vector<RGaussCoef> coefs;
  auto coef = [&](double sigma, double sp, int order) {
    auto key = std::make_tuple(sigma, sp, order);
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    coefs.push_back(rgauss_coefficients(sigma, sp, order, normalize != 0));
    return seen[key] = (int)coefs.size() - 1;
  };
  // the items class by class: a class is one launch over a contiguous range of the table
  std::vector<BatchLogItem> items;
  items.reserve((size_t)n_items);
  long long first[PRAD_BLOG_CLASSES + 1] = {0, 0, 0, 0}, lds[PRAD_BLOG_CLASSES] = {0, 0, 0};
  for (int k = 0; k < PRAD_BLOG_CLASSES; k++) {
    first[k] = (long long)items.size();
    for (int b = 0; b < B; b++) {
      if (cls[(size_t)b] != k) continue;
      for (int q = 0; q < S; q++) {
        if (verdict[(long long)q * B + b] != 0) continue;
        BatchLogItem it;
        it.roi = b;
        it.row = q;
        for (int d = 0; d < 3; d++) {
          it.c2[d] = coef(sigmas[q], spacing[3 * b + d], 2);
          it.c0[d] = coef(sigmas[q], spacing[3 * b + d], 0);
        }
        items.push_back(it);
        const long long f = blog_footprint(sizes + 3 * b);
        lds[k] = f > lds[k] ? f : lds[k];
      }
    }
  }
  first[PRAD_BLOG_CLASSES] = (long long)items.size();

  RecordTable<BatchLogRoi> recs;
  const size_t items_bytes = sizeof(BatchLogItem) * items.size();
  PRAD_TRY(recs.reserve(c, "batch_log_meta", (size_t)B, items_bytes + sizeof(RGaussCoef) * coefs.size()));
  for (int b = 0; b < B; b++) {
    BatchLogRoi &r = recs.host[b];
    r.off = off[b];
    r.nz = sizes[3 * b];
    r.ny = sizes[3 * b + 1];
    r.nx = sizes[3 * b + 2];
    r.pad = 0;
    for (int d = 0; d < 3; d++) r.sp2[d] = spacing[3 * b + d] * spacing[3 * b + d];
  }
  memcpy(recs.host_tail(), items.data(), items_bytes);
  memcpy((char *)recs.host_tail() + items_bytes, coefs.data(), sizeof(RGaussCoef) * coefs.size());
  const BatchLogItem *d_items = (const BatchLogItem *)recs.dev_tail();
  const RGaussCoef *d_coefs = (const RGaussCoef *)((const char *)recs.dev_tail() + items_bytes);
  return batch_call(c, s, recs, "batch-log", [&]() {
    Timed t(c, "batch_log", s);
    for (int k = 0; k < PRAD_BLOG_CLASSES; k++) {
      const long long n = first[k + 1] - first[k];
      if (n == 0) continue;
      PRAD_TRY(dispatch_image_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        const BatchLogItem *it = d_items + first[k];
        if (k == 0) return launch<T, PRAD_BLOG_THREADS_0>(c, s, (unsigned)n, (size_t)lds[k], in, recs.dev, it, d_coefs, out, row_stride);
        if (k == 1) return launch<T, PRAD_BLOG_THREADS_1>(c, s, (unsigned)n, (size_t)lds[k], in, recs.dev, it, d_coefs, out, row_stride);
        return launch<T, PRAD_BLOG_THREADS_2>(c, s, (unsigned)n, (size_t)lds[k], in, recs.dev, it, d_coefs, out, row_stride);
      }));
    }
    return (int)PRAD_OK;
  });
}
