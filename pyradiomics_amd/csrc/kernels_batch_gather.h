// kernels_batch_gather.h -- the door of the batched small-ROI route (gfx950): the boxes of MANY labels of one label map are
// copied out of a volume into the packed batch layout (kernels_batch_firstorder.h) in ONE launch.
//
// batch_gather_kernel<T, L>.  ROI b is the box [nz][ny][nx] whose first element lies at element `src` of the volume (row
// stride sy, plane stride sz); its n = nz ny nx elements go to element `off` .. off + n - 1 of the packed image buffer and of
// the packed uint8 mask buffer, the mask as labelmap == label (voxels of OTHER labels inside the box are outside the ROI).
//   work      the batch is a line of W = sum n work items, item w[b] + e being element e of ROI b; workgroup c takes the items
//             [c * PRAD_GATHER_CHUNK, (c + 1) * PRAD_GATHER_CHUNK), so a 60^3 box next to 300 boxes of 6^3 spreads over
//             211 workgroups instead of holding one for the whole launch.
//   lookup    first[c] (host-built, nchunks + 1 entries) is the ROI of the chunk's first item, first[c + 1] that of the next
//             chunk's (B - 1 behind the last chunk): a lane bisects w[] between the two -- no step inside a large box, three
//             for boxes of 6^3.  The records are read through the caches; every trip count follows from the tables alone.
//   lanes     lane t of 256 takes the items t, t + 256, t + 512, t + 768 of the chunk: consecutive lanes store consecutive
//             packed elements and load consecutive x of one box row until the row ends (rows here are 4 to 40 voxels: a lane
//             per row would leave most of a wave idle).
//   indices   items, offsets and volume positions are 64-bit; the split of e into (z, y, x) uses 32-bit divisions when the box
//             holds fewer than 2^32 voxels (one flag per record), 64-bit ones otherwise.
// T is an unsigned integer of the image's element width (values are moved, never interpreted: -0.0, NaN payloads and inf
// survive bit for bit) or GatherNone (masks only); L the label map's element type or GatherNone (images only).
#pragma once
#include "prad_runtime.h"

namespace prad {

#define PRAD_GATHER_THREADS 256
#define PRAD_GATHER_PER_LANE 4
#define PRAD_GATHER_CHUNK (PRAD_GATHER_THREADS * PRAD_GATHER_PER_LANE)

struct GatherNone {};

struct GatherRoi {
  long long w;     // first work item of the ROI (prefix sum of the box volumes)
  long long n;     // voxels of the box
  long long off;   // first element in the packed outputs
  long long src;   // element of the volume the box starts at
  int ny, nx;
  int label;
  int pad;
};
static_assert(sizeof(GatherRoi) == 48, "GatherRoi is uploaded as an array of 48-byte records");

template <typename T, typename L>
__global__ void __launch_bounds__(PRAD_GATHER_THREADS)
batch_gather_kernel(const T *__restrict__ image, const L *__restrict__ labelmap, const GatherRoi *__restrict__ rois,
                    const int *__restrict__ first, long long total, long long sy, long long sz, T *__restrict__ out_image,
                    unsigned char *__restrict__ out_mask) {
  const long long chunk = blockIdx.x;
  const int b_lo = first[chunk], b_hi = first[chunk + 1];
#pragma unroll
  for (int k = 0; k < PRAD_GATHER_PER_LANE; k++) {
    const long long item = chunk * PRAD_GATHER_CHUNK + (long long)k * PRAD_GATHER_THREADS + threadIdx.x;
    if (item >= total) break;
    int a = b_lo, z = b_hi;          // the last ROI of [b_lo, b_hi] with w <= item
    while (a < z) {
      const int m = (a + z + 1) >> 1;
      if (rois[m].w <= item) a = m;
      else z = m - 1;
    }
    const GatherRoi r = rois[a];
    const long long e = item - r.w;
    long long zz, yy, xx;
    if (r.n <= 0xffffffffLL) {
      const unsigned plane = (unsigned)r.ny * (unsigned)r.nx, e32 = (unsigned)e;
      const unsigned q = e32 / plane, rem = e32 - q * plane, y32 = rem / (unsigned)r.nx;
      zz = q;
      yy = y32;
      xx = rem - y32 * (unsigned)r.nx;
    } else {
      const long long plane = (long long)r.ny * r.nx;
      zz = e / plane;
      const long long rem = e - zz * plane;
      yy = rem / r.nx;
      xx = rem - yy * r.nx;
    }
    const long long from = r.src + zz * sz + yy * sy + xx, to = r.off + e;
    if constexpr (!std::is_same<T, GatherNone>::value) out_image[to] = image[from];
    if constexpr (!std::is_same<L, GatherNone>::value) out_mask[to] = (int)labelmap[from] == r.label ? 1 : 0;
  }
}

}  // namespace prad
