// kernels_lbp2d.h -- the LBP2D image type (imageoperations.py:1094-1166 on scikit-image's local_binary_pattern) of one volume
// in ONE launch (gfx950).  The volume is [nz][ny][nx] (TIN: int16 / int32 / float32 / float64, widened to float64: exact), the
// planes are stacked along `axis` (force2Ddimension; prad_lbp2d_plan.h names rows and cols per axis).
//
// Arithmetic, all float64, restated from scikit-image's published algorithm (DESIGN.md "LBP2D"): for the pixel (r, c) of a plane
// and sample i, y = r + rp[i], x = c + cp[i] with the HOST's table (rp, cp: no trigonometry here); minr = floor(y), maxr =
// ceil(y), minc = floor(x), maxc = ceil(x); dr = y - minr, dc = x - minc; a corner outside the plane reads 0.0;
//   top = (1 - dc) tl + dc tr      bottom = (1 - dc) bl + dc br      t_i = (1 - dr) top + dr bottom      s_i = t_i - centre >= 0
// Contraction is off (#pragma clang fp contract(off)): every product and every sum is rounded, no product is fused into a sum
// -- a flat neighbourhood of a level that is no small integer gives t_i one ulp off the centre, and the sign of that ulp is
// the code.  The full formula runs when dr or dc is 0, so NaN and infinities behave as in numpy.
//   uniform   changes = #{i in 0 .. P-2: s_i != s_{i+1}} (P - 1 pairs, not cyclic); sum s_i when changes <= 2, else P + 1
//   default   sum s_i 2^i                    ror   the minimum over the P cyclic rotations of that P-bit word
//
// lbp2d_tile_run   one workgroup, one tile of prad_lbp2d_plan.h: the staged block goes to LDS once, converted to float64, cells
//   beyond the volume as 0.0, x fastest (consecutive lanes load consecutive x: coalesced whatever the axis); after the barrier
//   lane t takes the output voxels t, t + 256, ... of the tile, x fastest again.  The offsets of a sample are uniform over the
//   wave, so its four corners are lane-consecutive float64 LDS reads (ds_read_b64, conflict-free) for every axis; with axis 2
//   the lanes run over the planes.  The kernels of this header and of kernels_batch_lbp2d.h both call it: a box of the batch
//   equals the single call bit for bit by construction.
// indices: voxel indices are 64-bit; LDS indices, tile coordinates and the in-tile splits (shifts: the extents are powers of
// two) are 32-bit.  |rp|, |cp| <= halo has been checked on the host, so floor(r + rp) >= r - halo and ceil(r + rp) <= r + halo
// (rounding is monotone and r +- halo is a float64): no LDS read leaves the staged block.  No atomics, no memset.
#pragma once
#include <type_traits>

#include "prad_lbp2d_plan.h"
#include "prad_runtime.h"

namespace prad {

#define PRAD_LBP_UNIFORM 0
#define PRAD_LBP_DEFAULT 1
#define PRAD_LBP_ROR 2

struct LbpTable {
  double rp[kLbpMaxSamples], cp[kLbpMaxSamples];
};

// the launch's geometry: by value in the kernel arguments (uniform: scalar registers)
struct LbpGeom {
  int tile[3];      // tz ty tx
  int lty, ltx;     // log2 ty, log2 tx
  int axis, halo, P, method;
};

inline LbpGeom lbp_geom(const Lbp2dPlan &p, int axis, int halo, int P, int method) {
  LbpGeom g;
  for (int d = 0; d < 3; d++) g.tile[d] = p.tile[d];
  g.lty = g.ltx = 0;
  while ((1 << g.lty) < p.tile[1]) g.lty++;
  while ((1 << g.ltx) < p.tile[2]) g.ltx++;
  g.axis = axis;
  g.halo = halo;
  g.P = P;
  g.method = method;
  return g;
}

#if defined(__HIPCC__)
template <typename TIN, typename TOUT>
__device__ __forceinline__ void lbp2d_tile_run(const TIN *__restrict__ in, TOUT *__restrict__ out, int nz, int ny, int nx, int z0,
                                               int y0, int x0, const LbpGeom &g, const LbpTable &tab, double *__restrict__ lds) {
#pragma clang fp contract(off)
  const int h = g.halo;
  const int hz = g.axis != 0 ? h : 0, hy = g.axis != 1 ? h : 0, hx = g.axis != 2 ? h : 0;
  const int ez = g.tile[0] + 2 * hz, ey = g.tile[1] + 2 * hy, ex = g.tile[2] + 2 * hx;
  const unsigned cells = (unsigned)(ez * ey * ex);
  for (unsigned c = threadIdx.x; c < cells; c += kLbpThreads) {
    const unsigned q = c / (unsigned)ex, lx = c - q * (unsigned)ex, lz = q / (unsigned)ey, ly = q - lz * (unsigned)ey;
    const int gz = z0 - hz + (int)lz, gy = y0 - hy + (int)ly, gx = x0 - hx + (int)lx;
    double v = 0.0;
    if (gz >= 0 && gz < nz && gy >= 0 && gy < ny && gx >= 0 && gx < nx) v = (double)in[((long long)gz * ny + gy) * nx + gx];
    lds[c] = v;
  }
  __syncthreads();
  // rows and cols of the plane as strides of the staged block, and as coordinates of the volume
  const int sz = ey * ex, sy = ex;
  const int rs = g.axis == 1 ? sz : sy, cs = g.axis == 2 ? sz : 1;
  const unsigned outs = (unsigned)(g.tile[0] << (g.lty + g.ltx));
  const unsigned P = (unsigned)g.P, full = P >= 32 ? 0xffffffffu : ((1u << P) - 1u);
  for (unsigned o = threadIdx.x; o < outs; o += kLbpThreads) {
    const int ox = (int)(o & (unsigned)(g.tile[2] - 1)), oy = (int)((o >> g.ltx) & (unsigned)(g.tile[1] - 1)),
              oz = (int)(o >> (g.ltx + g.lty));
    const int gz = z0 + oz, gy = y0 + oy, gx = x0 + ox;
    if (gz >= nz || gy >= ny || gx >= nx) continue;
    const int ci = (oz + hz) * sz + (oy + hy) * sy + (ox + hx);
    const int ri = g.axis == 1 ? gz : gy, cj = g.axis == 2 ? gz : gx;
    const double r = (double)ri, c = (double)cj, centre = lds[ci];
    unsigned bits = 0;
    for (unsigned i = 0; i < P; i++) {
      const double y = r + tab.rp[i], x = c + tab.cp[i];
      const double minr = floor(y), maxr = ceil(y), minc = floor(x), maxc = ceil(x);
      const double dr = y - minr, dc = x - minc;
      const int a0 = ci + ((int)minr - ri) * rs, a1 = ci + ((int)maxr - ri) * rs;
      const int b0 = ((int)minc - cj) * cs, b1 = ((int)maxc - cj) * cs;
      const double tl = lds[a0 + b0], tr = lds[a0 + b1], bl = lds[a1 + b0], br = lds[a1 + b1];
      const double top = (1.0 - dc) * tl + dc * tr;
      const double bottom = (1.0 - dc) * bl + dc * br;
      const double t = (1.0 - dr) * top + dr * bottom;
      bits |= (t - centre >= 0.0 ? 1u : 0u) << i;
    }
    unsigned code;
    if (g.method == PRAD_LBP_UNIFORM) {
      const unsigned changes = (unsigned)__popc((bits ^ (bits >> 1)) & (full >> 1));
      code = changes <= 2 ? (unsigned)__popc(bits) : P + 1;
    } else if (g.method == PRAD_LBP_DEFAULT) {
      code = bits;
    } else {
      code = bits;
      for (unsigned k = 1; k < P; k++) {
        const unsigned rot = ((bits >> k) | (bits << (P - k))) & full;
        code = rot < code ? rot : code;
      }
    }
    out[((long long)gz * ny + gy) * nx + gx] = (TOUT)code;
  }
}

// one workgroup per tile; block b is tile (b / (nty ntx), b / ntx % nty, b % ntx)
template <typename T>
__global__ void __launch_bounds__(kLbpThreads)
lbp2d_kernel(const T *__restrict__ in, T *__restrict__ out, int nz, int ny, int nx, unsigned nty, unsigned ntx, LbpGeom g,
             LbpTable tab) {
  extern __shared__ double lbp_lds[];
  const unsigned b = blockIdx.x, q = b / ntx, tx = b - q * ntx, tz = q / nty, ty = q - tz * nty;
  lbp2d_tile_run<T, T>(in, out, nz, ny, nx, (int)tz * g.tile[0], (int)ty * g.tile[1], (int)tx * g.tile[2], g, tab, lbp_lds);
}
#endif  // __HIPCC__

}  // namespace prad
