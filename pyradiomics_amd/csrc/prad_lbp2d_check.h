// prad_lbp2d_check.h -- the argument checks prad_lbp2d_dev and prad_batch_lbp2d_dev share; host only.
#pragma once
#include <math.h>

#include "kernels_lbp2d.h"

namespace prad {

static inline int lbp_size_check(const char *what, const int *size, int axis) {
  if (axis < 0 || axis > 2) return fail(PRAD_E_ARG, "%s: axis=%d outside 0 .. 2", what, axis);
  for (int d = 0; d < 3; d++)
    if (size[d] < 1) return fail(PRAD_E_ARG, "%s: size[%d]=%d < 1", what, d, size[d]);
  return PRAD_OK;
}

// dtype / out_dtype: image dtype codes (out_dtype 1 for the batch's float64 rows).  PRAD_E_UNSUPPORTED beyond the native domain
// (the caller takes the host route), PRAD_E_ARG for what no route computes.  Fills *tab.
static inline int lbp_args_check(const char *what, int dtype, int out_dtype, const double *rp, const double *cp, int P, int halo,
                                 int method, LbpTable *tab) {
  if (dtype < 0 || dtype > 3) return fail(PRAD_E_ARG, "%s: dtype %d", what, dtype);
  if (method < PRAD_LBP_UNIFORM || method > PRAD_LBP_ROR) return fail(PRAD_E_ARG, "%s: method %d (0 uniform, 1 default, 2 ror)", what, method);
  if (P < 1 || !rp || !cp) return fail(PRAD_E_ARG, "%s: P=%d, rp=%p, cp=%p", what, P, (const void *)rp, (const void *)cp);
  if (halo < 0) return fail(PRAD_E_ARG, "%s: halo=%d < 0", what, halo);
  if (P > kLbpMaxSamples || halo > kLbpMaxHalo)
    return fail(PRAD_E_UNSUPPORTED, "%s: P=%d, halo=%d beyond the native domain (P <= %d, halo <= %d)", what, P, halo, kLbpMaxSamples,
                kLbpMaxHalo);
  if (out_dtype == 3 && method != PRAD_LBP_UNIFORM && P > 15)
    return fail(PRAD_E_ARG, "%s: the codes of %d samples do not fit an int16 image", what, P);
  for (int i = 0; i < P; i++) {      // the kernel reads LDS at floor / ceil of r + rp: the table must stay within the halo
    if (!(fabs(rp[i]) <= (double)halo) || !(fabs(cp[i]) <= (double)halo))
      return fail(PRAD_E_ARG, "%s: sample %d at (%g, %g) lies beyond the halo %d", what, i, rp[i], cp[i], halo);
    tab->rp[i] = rp[i];
    tab->cp[i] = cp[i];
  }
  for (int i = P; i < kLbpMaxSamples; i++) tab->rp[i] = tab->cp[i] = 0.0;
  return PRAD_OK;
}

}  // namespace prad
