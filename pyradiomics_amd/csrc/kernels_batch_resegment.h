// kernels_batch_resegment.h -- resegmentation of B small boxes in ONE launch (prad_batch_resegment_dev): a workgroup per ROI
// walks its box once per pass -- statistics (relative, sigma), squared deviations (sigma), mask -- and writes the ROI's row: new
// mask, box and count of the kept ROI, thresholds, verdict.  The box is read from global memory / L2 in every pass (no LDS copy:
// a box of the cap is 64 K voxels), the reductions are those of the single call (kernels_resegment.h) with ONE partial, so a
// ROI's row depends on its values alone.  No atomics, no memset.
#pragma once
#include "kernels_resegment.h"

namespace prad {

struct BatchResegRoi {
  long long off;     // first element of the box in the packed image / masks
  int nz, ny, nx;
  int served;        // 0: above the cap, verdict 8 and nothing else written
};
static_assert(sizeof(BatchResegRoi) == 24, "BatchResegRoi is uploaded as an array of 24-byte records");

// what comes back per ROI
struct BatchResegRow {
  int box[7];        // lo z / y / x, hi z / y / x, count of the KEPT ROI (prad_batch_mask_boxes_dev's layout)
  int verdict;
  double thr[2];
};
static_assert(sizeof(BatchResegRow) == 48, "BatchResegRow is read back as an array of 48-byte records");

template <typename T>
__global__ void __launch_bounds__(PRAD_RESEG_THREADS)
batch_resegment_kernel(const T *__restrict__ image, const unsigned char *__restrict__ mask, const BatchResegRoi *__restrict__ rois,
                       ResegRange r, unsigned char *__restrict__ out_mask, BatchResegRow *__restrict__ rows) {
  __shared__ double scratch[PRAD_RESEG_WAVES];
  __shared__ int red[6][PRAD_RESEG_WAVES];
  const BatchResegRoi roi = rois[blockIdx.x];
  BatchResegRow *row = rows + blockIdx.x;
  const int t = threadIdx.x;
  if (!roi.served) {
    if (t == 0) {
      for (int k = 0; k < 7; k++) row->box[k] = 0;
      row->verdict = 8;
      row->thr[0] = row->thr[1] = 0.0;
    }
    return;
  }
  const unsigned n = (unsigned)roi.nz * (unsigned)roi.ny * (unsigned)roi.nx, plane = (unsigned)roi.ny * (unsigned)roi.nx;
  const T *img = image + roi.off;
  const unsigned char *m = mask + roi.off;
  unsigned char *out = out_mask + roi.off;

  // pass 1: the ROI's statistics (every mode: the count and the non-finite flag decide the verdict)
  long long count = 0;
  typename ResegSum<T>::type acc = 0;
  double top = -__builtin_inf();
  int bad = 0;
  for (unsigned e = t; e < n; e += PRAD_RESEG_THREADS) {
    if (m[e] == 0) continue;
    const T x = img[e];
    count++;
    acc += (typename ResegSum<T>::type)x;
    top = fmax(top, (double)x);
    bad |= !reseg_finite(x);
  }
  const ResegStats<T> s = reseg_block_stats<T>(count, acc, top, bad, scratch);
  const bool sigma32 = r.mode == PRAD_RESEG_SIGMA && std::is_same<T, float>::value;      // numpy's float32 mean: host route
  if (s.count == 0 || s.nonfinite || sigma32) {      // (uniform over the workgroup)
    for (unsigned e = t; e < n; e += PRAD_RESEG_THREADS) out[e] = 0;
    if (t == 0) {
      row->box[0] = roi.nz;
      row->box[1] = roi.ny;
      row->box[2] = roi.nx;
      row->box[3] = row->box[4] = row->box[5] = -1;
      row->box[6] = 0;
      row->verdict = s.count == 0 ? 1 : (s.nonfinite ? 2 : 8);
      row->thr[0] = row->thr[1] = 0.0;
    }
    return;
  }

  // pass 2 (sigma): squared deviations about the mean
  double dev2 = 0.0;
  if (r.mode == PRAD_RESEG_SIGMA) {
    const double mean = reseg_mean(s);
    double a = 0.0;
    for (unsigned e = t; e < n; e += PRAD_RESEG_THREADS) {
      if (m[e] == 0) continue;
      const double d = __dsub_rn((double)img[e], mean);
      a = __dadd_rn(a, __dmul_rn(d, d));
    }
    dev2 = reseg_block_sum<double>(a, scratch);
  }
  double thr[2];
  reseg_thresholds<T>(r, s, dev2, thr);

  // pass 3: the new mask, the kept count and its box
  int lo_z = roi.nz, lo_y = roi.ny, lo_x = roi.nx, hi_z = -1, hi_y = -1, hi_x = -1;
  long long kept = 0;
  for (unsigned e = t; e < n; e += PRAD_RESEG_THREADS) {
    unsigned char o = 0;
    if (m[e] != 0 && reseg_keep<T>(img[e], thr, r.two)) {
      o = 1;
      kept++;
      const unsigned z = e / plane, rem = e - z * plane, y = rem / (unsigned)roi.nx, x = rem - y * (unsigned)roi.nx;
      lo_z = min(lo_z, (int)z);
      lo_y = min(lo_y, (int)y);
      lo_x = min(lo_x, (int)x);
      hi_z = max(hi_z, (int)z);
      hi_y = max(hi_y, (int)y);
      hi_x = max(hi_x, (int)x);
    }
    out[e] = o;
  }
  kept = reseg_block_sum<long long>(kept, scratch);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo_z = min(lo_z, __shfl_xor(lo_z, o));
    lo_y = min(lo_y, __shfl_xor(lo_y, o));
    lo_x = min(lo_x, __shfl_xor(lo_x, o));
    hi_z = max(hi_z, __shfl_xor(hi_z, o));
    hi_y = max(hi_y, __shfl_xor(hi_y, o));
    hi_x = max(hi_x, __shfl_xor(hi_x, o));
  }
  if ((t & 63) == 0) {
    const int w = t >> 6;
    red[0][w] = lo_z;
    red[1][w] = lo_y;
    red[2][w] = lo_x;
    red[3][w] = hi_z;
    red[4][w] = hi_y;
    red[5][w] = hi_x;
  }
  __syncthreads();
  if (t < 6) {
    int v = red[t][0];
    for (int w = 1; w < PRAD_RESEG_WAVES; w++) v = t < 3 ? min(v, red[t][w]) : max(v, red[t][w]);
    row->box[t] = v;
  }
  if (t == 0) {
    row->box[6] = (int)kept;
    row->verdict = kept <= 1 ? 3 : 0;
    row->thr[0] = thr[0];
    row->thr[1] = thr[1];
  }
}

}  // namespace prad
