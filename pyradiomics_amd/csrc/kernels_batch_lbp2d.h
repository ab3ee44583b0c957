// kernels_batch_lbp2d.h -- the LBP2D images of MANY boxes in ONE launch (gfx950), on the batch layout of
// kernels_batch_firstorder.h: ROI b is the box [nz][ny][nx] at element `off` of the packed image (TIN: int16 / int32 / float32 /
// float64) and of the float64 output row.  Work is divided by output tiles from a host-built item table (prad_lbp2d_plan.h:
// batch_lbp2d_plan), one workgroup per item, boxes of any size; every workgroup runs lbp2d_tile_run of kernels_lbp2d.h on its
// box ALONE -- cells beyond the box's edge are 0.0 --, so a box equals the single call on it bit for bit.
#pragma once
#include "kernels_lbp2d.h"

namespace prad {

struct BatchLbpRoi {
  long long off;      // first element of the box in the packed image and in the output row
  int nz, ny, nx;
  int pad;
};
static_assert(sizeof(BatchLbpRoi) == 24, "BatchLbpRoi is uploaded as an array of 24-byte records");

#if defined(__HIPCC__)
template <typename TIN>
__global__ void __launch_bounds__(kLbpThreads)
batch_lbp2d_kernel(const TIN *__restrict__ in, double *__restrict__ out, const BatchLbpRoi *__restrict__ rois,
                   const BatchLbpItem *__restrict__ items, LbpGeom g, LbpTable tab) {
  extern __shared__ double lbp_lds[];
  const BatchLbpItem it = items[blockIdx.x];
  const BatchLbpRoi r = rois[it.roi];
  lbp2d_tile_run<TIN, double>(in + r.off, out + r.off, r.nz, r.ny, r.nx, it.z0, it.y0, it.x0, g, tab, lbp_lds);
}
#endif  // __HIPCC__

}  // namespace prad
