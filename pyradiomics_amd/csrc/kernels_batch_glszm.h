// kernels_batch_glszm.h -- the GLSZM zone lists and matrices of MANY small ROIs, one launch each (gfx950).
//
// The single GLSZM call (prad_glszm.hip) labels 256^3 .. 512^3 volumes with a tiled two-level union-find: tile kernel,
// dense init, pairs, root sum, stats, a read-back, the fill.  A lesion box of 10^3 .. 37^3 voxels fits in LDS whole, so here
// ONE workgroup of 256 threads labels a ROI completely on chip -- no tiles, no cross-tile pairs, no global forest.
//
// LDS budget of batch_glszm_kernel (dynamic, sized by the largest ROI of the batch; V = its voxels rounded up to 16):
//     PRAD_BZ_MISC_BYTES     256   verdict, three rotating "changed" flags, four wave totals, two reduction words
//   + V                            the packed ROI: one byte per voxel, 0 = outside the mask (the pack of batch_rois_kernel)
//   + 2 V                          a 16-bit label per voxel (a voxel index stays below 65536)
//   => PRAD_BATCH_GLSZM_MAX_VOX = (160 KiB - 256) / 3 = 54528 voxels (a multiple of 16; 37^3 = 50653 fits).  A ROI near the
//   cap takes a CU alone; a batch of 16^3 boxes asks for 12.3 KiB and runs 8 workgroups per CU (the 32-wave limit).
//
// Labelling.  label[v] starts as v.  A sweep replaces label[v] by the minimum of label[v], label[label[v]] (pointer jump)
// and the labels of the neighbours of v's level inside the box; sweeps repeat until one changes nothing.  The neighbourhood
// is a compile-time variant of the kernel (template argument F2D, the forced dimension of force2D): -1 the up to 26
// neighbours, 0 / 1 / 2 the up to 8 neighbours in the plane of the two other axes (z, y, x) -- the angle sets the single call
// is given.  The argument below holds for any symmetric neighbourhood, so for all four.
//   * There are no 16-bit LDS atomics and none are needed: a voxel's slot is written by its own thread only (ds_write_b16),
//     the other threads only read it, and a 16-bit LDS access is single-copy atomic -- a reader sees the old or the new label.
//   * Invariant: label[v] is the index of a voxel of v's zone and label[v] <= v (true at the start; every candidate of the
//     minimum is a label of a voxel of the same zone).  Labels only decrease, so a sweep that changes something lowers the
//     sum of all labels: the loop ends on every input.
//   * Fixed point: no label changes, so label[v] <= label[n] for every pair of neighbours of one level, in both directions:
//     labels are equal along every edge, hence constant on a zone.  The zone's smallest index m has label[m] = m (the
//     invariant leaves nothing smaller), so every voxel of the zone carries m -- the voxel at which the reference's raster
//     scan discovers the zone (cmatrices.c:255-258).
//   * Speed of convergence.  A thread owns a CONTIGUOUS range of voxels and walks it forwards in even sweeps, backwards in
//     odd ones, reading the labels it has just written (Gauss-Seidel): a label crosses a thread's whole range along x in one
//     sweep, in either direction.  The pointer jump doubles the reach along any path whose indices grow away from the zone's
//     first voxel.  What remains slow is a one-voxel-wide path that runs against the raster order along y or z: one voxel
//     per sweep.  A serpentine through all 54528 voxels of a 1 x 213 x 256 box is the test of that.
//     Forced x (F2D = 2): the neighbours lie in the (z, y) plane, so two consecutive voxels of a range are no neighbours
//     (unless nx = 1) and the Gauss-Seidel reach along x joins nothing; a label crosses a range only between the rows of the
//     range that lie above one another (ranges longer than nx).  A straight line along y or z is left to the pointer jump: its
//     indices grow away from the zone's first voxel, O(log length) sweeps.  The slow path is now EVERY one-voxel-wide path
//     that runs against the raster order, whichever its direction in the plane -- e.g. the rising arm of a U: one voxel per
//     sweep, at most the nz * ny voxels of one x-plane.  Forced z and forced y keep the reach along x and the slow path of
//     the unforced kernel, confined to one plane.
//   * LDS traffic.  Labels are read as ds_read_u16 and levels as ds_read_u8 through address_space(3) pointers (through a
//     generic volatile pointer the compiler emits flat loads: kernels_glszm_labels.h, lds_find).  Banks are 4 bytes wide, 32 of them
//     for these instructions: with a range of `chunk` voxels per thread, lane l reads label bytes 2 * chunk * l + const, so
//     chunk = 2 (mod 4) -- an odd number of dwords -- puts the 32 lanes of a half wave on 32 different banks; the level bytes
//     of two neighbouring lanes then share a bank at most two ways.  Ranges above 8 voxels are rounded up to such a length.
//
// Zone list.  Roots (label[v] == v) are counted per thread range and ranked by a workgroup scan, which is the raster order of
// each zone's first voxel.  Zone sizes are summed with global atomics in the ROI's own zone-list region (ints nvox .. 2 nvox
// - 1, zeroed by this launch for the roots; a thread adds a run of voxels of one root at once), moved into the label slots
// of the roots, and only then are the (level, size) pairs written to ints 0 .. 2 nzones - 1 of the region.  The tail of
// the region beyond the pairs holds scratch values.  The distinct sizes are counted in a bitmap that reuses the level bytes.
//
// batch_glszm_fill_kernel histograms a ROI's zone list into float64, Ng the ROI's own count, dense [Ng][max(maxRegion, 1)] or
// compact [Ng][max(k, 1)] + the k distinct sizes ascending; every element of the slice is written by the ROI's workgroup.
#pragma once
#include "prad_runtime.h"

namespace prad {

#define PRAD_BZ_THREADS 256
#define PRAD_BZ_MAX_NG 64
#define PRAD_BZ_MISC_BYTES 256
#define PRAD_BATCH_GLSZM_MAX_VOX 54528
#define PRAD_BATCH_GLSZM_BITMAP_WORDS (PRAD_BATCH_GLSZM_MAX_VOX / 32 + 1)      // bits 0 .. MAX_VOX: a zone size is a bit index

static_assert(PRAD_BZ_MISC_BYTES + 3 * PRAD_BATCH_GLSZM_MAX_VOX == 160 * 1024, "misc + level bytes + 16-bit labels fill the LDS of a CU");
static_assert(PRAD_BATCH_GLSZM_MAX_VOX % 16 == 0, "ROI bytes are rounded up to 16");
static_assert(PRAD_BATCH_GLSZM_MAX_VOX <= 65536, "a voxel index and a zone size fit 16 bits");
static_assert(37 * 37 * 37 <= PRAD_BATCH_GLSZM_MAX_VOX, "a 37^3 box is covered");
static_assert(PRAD_BZ_THREADS == 256, "four waves: the scan keeps four wave totals");
static_assert(4 * 16 <= PRAD_BZ_MISC_BYTES, "misc block layout");

typedef __attribute__((address_space(3))) unsigned char bz_lds_u8;
typedef __attribute__((address_space(3))) unsigned short bz_lds_u16;
typedef __attribute__((address_space(3))) unsigned bz_lds_u32;

struct BatchZoneRoi {
  long long off;       // first element of the ROI in the level / mask buffers; its zone list starts at int 2 * off
  int nz, ny, nx;
  int Ng;              // the ROI's own grey-level count: its masked levels lie in [1, Ng]
};

struct BatchZoneArgs {
  const int32_t *levels;
  const uint8_t *mask;
  const BatchZoneRoi *rois;
  int vox_bytes;       // voxels of the largest ROI, rounded up to 16: bytes of the level region, half the bytes of the labels
  int *zones, *summary, *status;
};

// misc block (u32 words)
#define PRAD_BZ_BAD 0
#define PRAD_BZ_CHANGED 1      // 1 .. 3: sweep s raises word 1 + s % 3 and clears the word of sweep s + 1
#define PRAD_BZ_WAVES 4        // 4 .. 7
#define PRAD_BZ_MAX 8
#define PRAD_BZ_DISTINCT 9

// exclusive prefix sum of `v` over the 256 threads (in thread order) and the total; `waves`: four LDS words
__device__ __forceinline__ int bz_block_scan(int v, volatile bz_lds_u32 *waves, int *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  __syncthreads();             // (the words may still be read from an earlier scan)
  if (lane == 63) waves[w] = (unsigned)inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int t = (int)waves[k];
    if (k < w) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

template <int F2D>
__global__ void __launch_bounds__(PRAD_BZ_THREADS) batch_glszm_kernel(BatchZoneArgs A) {
  static_assert(F2D >= -1 && F2D <= 2, "forced dimension: none, z, y or x");
  extern __shared__ __align__(16) unsigned char bz_lds[];
  volatile bz_lds_u32 *misc = (volatile bz_lds_u32 *)bz_lds;
  bz_lds_u8 *L = (bz_lds_u8 *)(bz_lds + PRAD_BZ_MISC_BYTES);
  volatile bz_lds_u16 *lab = (volatile bz_lds_u16 *)(bz_lds + PRAD_BZ_MISC_BYTES + A.vox_bytes);

  const int tid = threadIdx.x, nthr = PRAD_BZ_THREADS;
  const int b = (int)blockIdx.x;
  const BatchZoneRoi R = A.rois[b];
  const int Ng = R.Ng, nx = R.nx, ny = R.ny, nz = R.nz;
  const int plane = ny * nx, nvox = nz * plane;
  int *zl = A.zones + 2 * R.off;      // the ROI's region: 2 * nvox ints
  int *scr = zl + nvox;               // zone sizes by root voxel, until the pairs are written

  // ---- pack (as batch_rois_kernel): one byte per voxel, 0 outside the mask; every voxel its own label -----------------------
  if (tid < 16) misc[tid] = 0;
  __syncthreads();
  {
    const int32_t *lv = A.levels + R.off;
    const uint8_t *mk = A.mask + R.off;
    bool bad = false;
    for (int i = tid; i < nvox; i += nthr) {
      int v = mk[i] ? lv[i] : 0;
      if (mk[i] && (v < 1 || v > Ng)) {
        bad = true;
        v = 0;
      }
      L[i] = (unsigned char)v;
      lab[i] = (unsigned short)i;
    }
    if (bad) misc[PRAD_BZ_BAD] = 1;
  }
  __syncthreads();
  if (misc[PRAD_BZ_BAD]) {   // the reference's IndexError: the ROI is void
    if (tid == 0) {
      A.status[b] = PRAD_INDEX_ERROR;
      A.summary[3 * b] = A.summary[3 * b + 1] = A.summary[3 * b + 2] = 0;
    }
    return;
  }

  // ---- the thread's contiguous range --------------------------------------------------------------------------------------------
  int chunk = (nvox + nthr - 1) / nthr;
  if (chunk > 8) chunk += (6 - (chunk & 3)) & 3;      // 2 (mod 4): see the bank note above
  const int v0 = min(nvox, tid * chunk), v1 = min(nvox, v0 + chunk);

  // ---- sweeps -------------------------------------------------------------------------------------------------------------------
  for (int sweep = 0;; sweep++) {
    if (tid == 0) misc[PRAD_BZ_CHANGED + (sweep + 1) % 3] = 0;
    bool changed = false;
    if (v0 < v1) {
      const bool fwd = !(sweep & 1);
      int v = fwd ? v0 : v1 - 1;
      int z = v / plane, r = v - z * plane, y = r / nx, x = r - y * nx;
      for (int n = v0; n < v1; n++) {
        const unsigned c = L[v];
        if (c) {
          const unsigned cur = lab[v];
          unsigned m = min(cur, (unsigned)lab[cur]);
#pragma unroll
          for (int dz = -1; dz <= 1; dz++) {
            if ((F2D == 0 && dz) || (unsigned)(z + dz) >= (unsigned)nz) continue;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
              if ((F2D == 1 && dy) || (unsigned)(y + dy) >= (unsigned)ny) continue;
              const int row = v + dz * plane + dy * nx;
#pragma unroll
              for (int dx = -1; dx <= 1; dx++) {
                if ((F2D == 2 && dx) || !(dz | dy | dx) || (unsigned)(x + dx) >= (unsigned)nx) continue;
                if (L[row + dx] == c) m = min(m, (unsigned)lab[row + dx]);
              }
            }
          }
          if (m < cur) {
            lab[v] = (unsigned short)m;
            changed = true;
          }
        }
        if (fwd) {
          v++;
          if (++x == nx) {
            x = 0;
            if (++y == ny) y = 0, z++;
          }
        } else {
          v--;
          if (--x < 0) {
            x = nx - 1;
            if (--y < 0) y = ny - 1, z--;
          }
        }
      }
    }
    if (changed) misc[PRAD_BZ_CHANGED + sweep % 3] = 1;
    __syncthreads();
    if (!misc[PRAD_BZ_CHANGED + sweep % 3]) break;      // (the same word for every thread: it is cleared again in sweep + 2)
  }

  // ---- zone sizes: summed at the root's scratch word -------------------------------------------------------------------------------
  int roots = 0;
  for (int v = v0; v < v1; v++)
    if (L[v] && lab[v] == v) {
      scr[v] = 0;
      roots++;
    }
  __threadfence();
  __syncthreads();
  {
    int root = -1, run = 0;
    for (int v = v0; v < v1; v++) {
      if (!L[v]) continue;
      const int r = lab[v];
      if (r != root) {
        if (run) atomicAdd(&scr[root], run);
        root = r, run = 0;
      }
      run++;
    }
    if (run) atomicAdd(&scr[root], run);
  }
  __threadfence();
  __syncthreads();
  // the label slot of a root takes its zone's size (<= nvox < 65536), every other slot 0
  unsigned largest = 0;
  for (int v = v0; v < v1; v++) {
    unsigned size = 0;
    if (L[v] && lab[v] == v) size = (unsigned)atomicAdd(&scr[v], 0);      // (read where the atomics landed)
    lab[v] = (unsigned short)size;
    largest = max(largest, size);
  }
  if (largest) atomicMax((unsigned *)bz_lds + PRAD_BZ_MAX, largest);
  int nzones = 0;
  int rank = bz_block_scan(roots, misc + PRAD_BZ_WAVES, &nzones);      // (its barriers: every scratch word has been read)

  // ---- the zone list, in raster order of each zone's first voxel --------------------------------------------------------------------
  for (int v = v0; v < v1; v++) {
    const int size = lab[v];
    if (size) {
      zl[2 * rank] = L[v];
      zl[2 * rank + 1] = size;
      rank++;
    }
  }
  __syncthreads();

  // ---- distinct sizes: a bitmap over 0 .. nvox in the bytes the levels held ----------------------------------------------------------
  unsigned *bitmap = reinterpret_cast<unsigned *>(bz_lds + PRAD_BZ_MISC_BYTES);
  const int words = nvox / 32 + 1;                     // 4 * words <= the 16-byte multiple above nvox
  for (int k = tid; k < words; k += nthr) bitmap[k] = 0;
  __syncthreads();
  for (int v = v0; v < v1; v++) {
    const unsigned size = lab[v];
    if (size) atomicOr(&bitmap[size >> 5], 1u << (size & 31));
  }
  __syncthreads();
  int distinct = 0;
  for (int k = tid; k < words; k += nthr) distinct += __popc(bitmap[k]);
  if (distinct) atomicAdd((unsigned *)bz_lds + PRAD_BZ_DISTINCT, (unsigned)distinct);
  __syncthreads();
  if (tid == 0) {
    A.summary[3 * b] = nzones;
    A.summary[3 * b + 1] = (int)misc[PRAD_BZ_MAX];
    A.summary[3 * b + 2] = (int)misc[PRAD_BZ_DISTINCT];
    A.status[b] = PRAD_OK;
  }
}

struct BatchFillRoi {
  long long zones;     // first int of the ROI's zone list
  long long out;       // first double of its matrix
  long long sizes;     // first int of its distinct sizes (compact)
  int nzones, max_region, nsizes;
  int Ng;              // rows of the ROI's matrix
};

// One workgroup per ROI.  A pair outside [1, Ng] x [1, max_region], or a size beyond the nsizes columns, is skipped: the
// records come from the summary the labelling launch wrote, a caller that passes another cannot make the kernel write
// outside the ROI's slice.
__global__ void __launch_bounds__(PRAD_BZ_THREADS) batch_glszm_fill_kernel(const int *__restrict__ zones,
                                                                              const BatchFillRoi *__restrict__ rois, int compact,
                                                                              double *out, int *sizes_out) {
  __shared__ unsigned bitmap[PRAD_BATCH_GLSZM_BITMAP_WORDS];
  __shared__ unsigned before[PRAD_BATCH_GLSZM_BITMAP_WORDS];      // set bits in the words below
  __shared__ unsigned waves[4];
  const int tid = threadIdx.x, nthr = PRAD_BZ_THREADS;
  const BatchFillRoi R = rois[blockIdx.x];
  const int Ng = R.Ng;
  const int *zl = zones + R.zones;
  const int cols = max(compact ? R.nsizes : R.max_region, 1);
  double *o = out + R.out;
  for (long long k = tid; k < (long long)Ng * cols; k += nthr) o[k] = 0.0;
  if (compact) {
    const int words = R.max_region / 32 + 1;
    for (int k = tid; k < words; k += nthr) bitmap[k] = 0;
    __syncthreads();
    for (int i = tid; i < R.nzones; i += nthr) {
      const int size = zl[2 * i + 1];
      if (size >= 1 && size <= R.max_region) atomicOr(&bitmap[size >> 5], 1u << (size & 31));
    }
    __syncthreads();
    const int per = (words + nthr - 1) / nthr, w0 = min(words, tid * per), w1 = min(words, w0 + per);
    int mine = 0, total = 0;
    for (int k = w0; k < w1; k++) mine += __popc(bitmap[k]);
    int rank = bz_block_scan(mine, (volatile bz_lds_u32 *)waves, &total);
    for (int k = w0; k < w1; k++) {
      before[k] = (unsigned)rank;
      for (unsigned bits = bitmap[k]; bits; bits &= bits - 1) {
        if (rank < R.nsizes) sizes_out[R.sizes + rank] = 32 * k + __ffs((int)bits) - 1;
        rank++;
      }
    }
  }
  __threadfence();       // the zeros are in place before the first increment
  __syncthreads();
  for (int i = tid; i < R.nzones; i += nthr) {
    const int level = zl[2 * i], size = zl[2 * i + 1];
    if (level < 1 || level > Ng || size < 1 || size > R.max_region) continue;
    const int col = compact ? (int)(before[size >> 5] + __popc(bitmap[size >> 5] & ((1u << (size & 31)) - 1u))) : size - 1;
    if (col < cols) atomicAdd(&o[(size_t)(level - 1) * cols + col], 1.0);
  }
}

}  // namespace prad
