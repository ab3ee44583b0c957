// prad_lbp2d.hip -- C ABI of the LBP2D image type of one volume (include/pyradiomics_amd.h: prad_lbp2d_plan, prad_lbp2d_dev);
// translation unit of libpyradiomics_amd.so.
#include <math.h>

#include "kernels_lbp2d.h"
#include "prad_batch_common.h"
#include "prad_lbp2d_check.h"

using namespace prad;

namespace {

template <typename T>
int launch(Context &c, hipStream_t s, const Lbp2dPlan &p, const LbpGeom &g, const LbpTable &tab, const void *in, void *out,
           const int *size) {
  Timed t(c, "lbp2d", s);
  hipLaunchKernelGGL(lbp2d_kernel<T>, dim3((unsigned)p.groups), dim3(kLbpThreads), (size_t)p.lds, s, (const T *)in, (T *)out,
                     size[0], size[1], size[2], (unsigned)p.tiles[1], (unsigned)p.tiles[2], g, tab);
  return check_launch("lbp2d_kernel");
}

}  // namespace

extern "C" int prad_lbp2d_plan(const int *size, int axis, int halo, int *tile, long long *grid, long long *lds_bytes, int *verdict) {
  if (!size || !tile || !grid || !lds_bytes || !verdict) return fail(PRAD_E_ARG, "lbp2d plan: NULL pointer");
  PRAD_TRY(lbp_size_check("lbp2d plan", size, axis));
  const Lbp2dPlan p = lbp2d_plan(size, axis, halo);
  for (int d = 0; d < 3; d++) {
    tile[d] = p.tile[d];
    grid[d] = p.tiles[d];
  }
  grid[3] = p.groups;
  *lds_bytes = p.lds;
  *verdict = p.verdict;
  return PRAD_OK;
}

extern "C" int prad_lbp2d_dev(const void *in, int dtype, const int *size, int axis, const double *rp, const double *cp, int P,
                              int halo, int method, void *out, void *stream) {
  if (!in || !out || !size) return fail(PRAD_E_ARG, "lbp2d: NULL pointer");
  if (in == out) return fail(PRAD_E_ARG, "lbp2d: the image cannot be filtered in place");
  PRAD_TRY(lbp_size_check("lbp2d", size, axis));
  LbpTable tab;
  PRAD_TRY(lbp_args_check("lbp2d", dtype, dtype, rp, cp, P, halo, method, &tab));
  const Lbp2dPlan p = lbp2d_plan(size, axis, halo);
  if (p.verdict != kLbpNative)
    return fail(PRAD_E_UNSUPPORTED, "lbp2d: %s", p.verdict == kLbpGrid ? "more workgroups than one launch holds" : "no tile fits the LDS budget");
  Context &c = ctx();
  PRAD_TRY(c.ensure_device());
  hipStream_t s = (hipStream_t)stream;
  const LbpGeom g = lbp_geom(p, axis, halo, P, method);
  PRAD_TRY(c.begin_call(s));
  const int rc = dispatch_image_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch<T>(c, s, p, g, tab, in, out, size);
  });
  PRAD_TRY(c.end_call(s));
  PRAD_TRY(rc);
  c.last_path = "lbp2d";
  c.last_variant = axis == 0 ? "lbp2d-axis0" : axis == 1 ? "lbp2d-axis1" : "lbp2d-axis2";
  return PRAD_OK;
}
