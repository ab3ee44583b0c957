// kernels_batch.h -- the texture matrices of MANY small ROIs in one launch (gfx950).
//
// A lesion-level study has thousands of ROIs whose boxes hold 10^3 .. 40^3 voxels.  The single-segment kernels have next to
// nothing to do on such a box: a call costs its launches.  Here one workgroup owns one (ROI, job): it packs the ROI -- int32
// levels + uint8 mask -> one byte per voxel, 0 = outside the mask -- into LDS, accumulates u32 tables in LDS and writes the
// float64 matrix slice it owns, zeros included, in the layout of the single calls.  No global atomics, no memset, no
// finalize launch: every output element has exactly one writer.
//
//   job kind      owns                                               table in LDS (u32)
//   GLCM group    a contiguous range of the ROI's angles             [angles at once][Ng][Ng]
//   GLRLM group   a contiguous range of the ROI's distance-1 angles  [angles at once][Ng][run-length columns at once]
//   neighbours    GLDM and NGTDM of the ROI (one neighbourhood scan) [levels at once][Nb + 1] dependence counts, then the
//                                                                    same shape of sum |c * level - sum(neighbours)| per
//                                                                    neighbour count c (NGTDM as kernels_neigh.h forms it)
// A table larger than the budget is built in passes (run-length columns r0 .. r0 + RC for GLRLM -- a 1 x 1 x N box has
// Nr = N --, levels l0 .. l0 + LC for GLDM / NGTDM with several distances); the common shapes take one pass.
//
// LDS budget.  The CU has 160 KiB; two resident workgroups get 81920 bytes each:
//     PRAD_BATCH_MISC_BYTES   256   verdict word, per-angle "a line holds two voxels" flags, the angles of the sub-batch
//   + PRAD_BATCH_TABLE_BYTES 16384  the largest table that must exist whole: one GLCM angle at 64 levels = 64 * 64 * 4
//   + the ROI's bytes
//   => PRAD_BATCH_MAX_VOX = 81920 - 16384 - 256 = 65280 voxels (a multiple of 16; 40^3 = 64000 fits).
// Smaller batches ask for less (largest ROI of the batch, the largest table any ROI asks for with its own Ng), so small ROIs
// run many workgroups per CU.  Every ROI carries its own Ng (BatchRoi.Ng): a workgroup sizes its passes from table_words / Ng.
// Table counts stay below 2^32: a count is at most the voxels of the ROI; an NGTDM slot adds at most Nb * 63 per voxel,
// 65280 * 254 * 63 < 2^30 -- hence PRAD_BATCH_MAX_NA (unidirectional angles; Nb = 2 Na neighbours).
#pragma once
#include "prad_runtime.h"

namespace prad {

#define PRAD_BATCH_THREADS 256
#define PRAD_BATCH_MAX_NG 64
#define PRAD_BATCH_MISC_BYTES 256
#define PRAD_BATCH_TABLE_BYTES 16384
#define PRAD_BATCH_MAX_VOX 65280
#define PRAD_BATCH_MAX_NA 127
#define PRAD_BATCH_ANGLES_AT_ONCE 8     // angles of one pass over the voxels (their offsets and flags live in the misc block)

static_assert(PRAD_BATCH_MISC_BYTES + PRAD_BATCH_TABLE_BYTES + PRAD_BATCH_MAX_VOX <= 160 * 1024 / 2, "two workgroups per CU");
static_assert(PRAD_BATCH_TABLE_BYTES >= 4 * PRAD_BATCH_MAX_NG * PRAD_BATCH_MAX_NG, "one GLCM angle");
static_assert(PRAD_BATCH_MAX_VOX % 16 == 0, "ROI bytes are rounded up to 16");
static_assert(4 * (16 + 3 * PRAD_BATCH_ANGLES_AT_ONCE) <= PRAD_BATCH_MISC_BYTES, "misc block layout");

struct BatchRoi {
  long long off;       // first element of the ROI in the level / mask buffers
  long long out[4];    // first double of the ROI in the GLCM / GLRLM / GLDM / NGTDM buffers
  int nz, ny, nx;
  int na, na_run;      // unidirectional angles of the requested distances (GLCM; GLDM / NGTDM use them in both directions)
                       // and of distance 1 (GLRLM)
  int ang, ang_run;    // their first row in the angle table (rows of 3 ints: dz, dy, dx)
  int Ng;              // the ROI's own grey-level count: its matrices have Ng rows and its masked levels lie in [1, Ng]
};

struct BatchArgs {
  const int32_t *levels;
  const uint8_t *mask;
  const BatchRoi *rois;
  const int *angles;
  int alpha;
  int groups_glcm, groups_glrlm, neigh;   // jobs per ROI: GLCM angle groups, GLRLM angle groups, 0 / 1 neighbourhood job
  int table_words;                        // u32 words of the table region (<= PRAD_BATCH_TABLE_BYTES / 4; at least Ng * Ng and
                                          // 2 * (2 na + 1) of every ROI: its smallest whole table)
  double *glcm, *glrlm, *gldm, *ngtdm;    // NULL: family not asked for
  int *status;
};

// misc block (u32 words): [0] verdict, [1 .. 8] per angle of the sub-batch "a line holds >= 2 masked voxels", [16 ..] its offsets
#define PRAD_BATCH_MISC_MULTI 1
#define PRAD_BATCH_MISC_ANGLES 16

__global__ void __launch_bounds__(PRAD_BATCH_THREADS) batch_rois_kernel(BatchArgs A) {
  extern __shared__ __align__(16) unsigned char batch_lds[];
  unsigned *misc = reinterpret_cast<unsigned *>(batch_lds);
  int *angs = reinterpret_cast<int *>(batch_lds) + PRAD_BATCH_MISC_ANGLES;
  unsigned *T = reinterpret_cast<unsigned *>(batch_lds + PRAD_BATCH_MISC_BYTES);
  uint8_t *L = batch_lds + PRAD_BATCH_MISC_BYTES + 4 * (size_t)A.table_words;

  const int tid = threadIdx.x, nthr = PRAD_BATCH_THREADS;
  const int jobs = A.groups_glcm + A.groups_glrlm + A.neigh;
  const int b = (int)(blockIdx.x / (unsigned)jobs), job = (int)(blockIdx.x % (unsigned)jobs);
  const BatchRoi R = A.rois[b];
  const int Ng = R.Ng, nx = R.nx, ny = R.ny, nz = R.nz;   // (all from the workgroup's one record: uniform, so the pass splits are)
  const int plane = ny * nx, nvox = nz * plane;

  // ---- pack: one byte per voxel, 0 outside the mask; a masked level outside [1, Ng] is the reference's IndexError ----------
  if (tid == 0) misc[0] = 0;
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
      L[i] = (uint8_t)v;
    }
    if (bad) misc[0] = 1;
  }
  __syncthreads();
  const bool bad = misc[0] != 0;
  if (job == 0 && tid == 0) A.status[b] = bad ? PRAD_INDEX_ERROR : PRAD_OK;
  if (bad) {   // its matrices are void: all jobs of the ROI write the matrices of an empty mask
    for (int i = tid; i < nvox; i += nthr) L[i] = 0;
    __syncthreads();
  }

  if (job < A.groups_glcm) {
    // ---- GLCM (cmatrices.c:4-92): ordered pairs (p, p + angle), both masked ---------------------------------------------
    const int na = R.na, per = (na + A.groups_glcm - 1) / A.groups_glcm;
    const int a0 = job * per, a1 = min(na, a0 + per);
    const int cells = Ng * Ng;
    const int at = max(1, min(PRAD_BATCH_ANGLES_AT_ONCE, A.table_words / cells));
    double *out = A.glcm + R.out[0];
    for (int s0 = a0; s0 < a1; s0 += at) {
      const int nt = min(at, a1 - s0);
      __syncthreads();
      for (int k = tid; k < nt * cells; k += nthr) T[k] = 0;
      for (int k = tid; k < 3 * nt; k += nthr) angs[k] = A.angles[(size_t)(R.ang + s0) * 3 + k];
      __syncthreads();
      for (int i = tid; i < nvox; i += nthr) {
        const int c = L[i];
        if (!c) continue;
        const int z = i / plane, r = i - z * plane, y = r / nx, x = r - y * nx;
        for (int t = 0; t < nt; t++) {
          const int zz = z + angs[3 * t], yy = y + angs[3 * t + 1], xx = x + angs[3 * t + 2];
          if ((unsigned)zz >= (unsigned)nz || (unsigned)yy >= (unsigned)ny || (unsigned)xx >= (unsigned)nx) continue;
          const int v = L[zz * plane + yy * nx + xx];
          if (v) atomicAdd(&T[(t * Ng + c - 1) * Ng + v - 1], 1u);
        }
      }
      __syncthreads();
      for (int k = tid; k < nt * cells; k += nthr) {   // [i][j][a]: the nt angles of a cell are adjacent doubles
        const int cell = k / nt, t = k - cell * nt;
        out[(size_t)cell * na + s0 + t] = (double)T[t * cells + cell];
      }
    }
    return;
  }

  if (job < A.groups_glcm + A.groups_glrlm) {
    // ---- GLRLM (cmatrices.c:299-541): a masked voxel whose predecessor along the angle is outside the box, outside the mask
    // or of another level opens a run and walks it.  Column 0 of an angle is cleared when none of its lines holds two
    // masked voxels (cmatrices.c:524-534): the first masked voxel of a line always opens a run, so it looks ahead. --------
    const int g = job - A.groups_glcm;
    const int na = R.na_run, per = (na + A.groups_glrlm - 1) / A.groups_glrlm;
    const int a0 = g * per, a1 = min(na, a0 + per);
    const int Nr = max(nz, max(ny, nx));
    const int RC = min(Nr, A.table_words / Ng);                      // run-length columns of one pass
    const int at = max(1, min(PRAD_BATCH_ANGLES_AT_ONCE, A.table_words / (Ng * RC)));
    double *out = A.glrlm + R.out[1];
    for (int s0 = a0; s0 < a1; s0 += at) {
      const int nt = min(at, a1 - s0);
      __syncthreads();
      for (int k = tid; k < 3 * nt; k += nthr) angs[k] = A.angles[(size_t)(R.ang_run + s0) * 3 + k];
      for (int k = tid; k < nt; k += nthr) misc[PRAD_BATCH_MISC_MULTI + k] = 0;
      __syncthreads();
      int longest = 0;   // voxels of the longest line of these angles: no run is longer
      for (int t = 0; t < nt; t++) {
        int len = Nr;
        if (angs[3 * t]) len = min(len, (nz + abs(angs[3 * t]) - 1) / abs(angs[3 * t]));
        if (angs[3 * t + 1]) len = min(len, (ny + abs(angs[3 * t + 1]) - 1) / abs(angs[3 * t + 1]));
        if (angs[3 * t + 2]) len = min(len, (nx + abs(angs[3 * t + 2]) - 1) / abs(angs[3 * t + 2]));
        longest = max(longest, len);
      }
      for (int r0 = 0; r0 < Nr; r0 += RC) {
        const int rc = min(RC, Nr - r0);
        const bool walk = r0 < longest;
        if (walk) {
          __syncthreads();
          for (int k = tid; k < nt * Ng * RC; k += nthr) T[k] = 0;
          __syncthreads();
          for (int i = tid; i < nvox; i += nthr) {
            const int c = L[i];
            if (!c) continue;
            const int z = i / plane, r = i - z * plane, y = r / nx, x = r - y * nx;
            for (int t = 0; t < nt; t++) {
              const int dz = angs[3 * t], dy = angs[3 * t + 1], dx = angs[3 * t + 2];
              const int step = dz * plane + dy * nx + dx;
              int zz = z - dz, yy = y - dy, xx = x - dx;
              int prev = 0;
              if ((unsigned)zz < (unsigned)nz && (unsigned)yy < (unsigned)ny && (unsigned)xx < (unsigned)nx) prev = L[i - step];
              if (prev == c) continue;                      // inside a run
              int len = 1, q = i + step;
              zz = z + dz, yy = y + dy, xx = x + dx;
              while ((unsigned)zz < (unsigned)nz && (unsigned)yy < (unsigned)ny && (unsigned)xx < (unsigned)nx && L[q] == c) {
                len++;
                q += step, zz += dz, yy += dy, xx += dx;
              }
              volatile unsigned *multi = misc + PRAD_BATCH_MISC_MULTI + t;
              if (!*multi) {
                bool two = prev != 0 || len > 1;
                while (!two && (unsigned)zz < (unsigned)nz && (unsigned)yy < (unsigned)ny && (unsigned)xx < (unsigned)nx) {
                  two = L[q] != 0;
                  q += step, zz += dz, yy += dy, xx += dx;
                }
                if (two) *multi = 1;
              }
              const int rl = len - 1 - r0;
              if (rl >= 0 && rl < rc) atomicAdd(&T[(t * Ng + c - 1) * RC + rl], 1u);
            }
          }
          __syncthreads();
        }
        for (int k = tid; k < nt * Ng * rc; k += nthr) {   // [g][r][a]
          const int cell = k / nt, t = k - cell * nt;
          const int gl = cell / rc, r = cell - gl * rc;
          unsigned v = walk ? T[(t * Ng + gl) * RC + r] : 0u;
          if (r0 + r == 0 && !misc[PRAD_BATCH_MISC_MULTI + t]) v = 0;
          out[((size_t)gl * Nr + r0 + r) * na + s0 + t] = (double)v;
        }
      }
    }
    return;
  }

  // ---- GLDM (cmatrices.c:660-754) and NGTDM (cmatrices.c:543-658) from one scan of the Nb = 2 na neighbours ------------------
  {
    const int na = R.na, Nb = 2 * na, W = Nb + 1, width = 2 * Nb + 1;
    const int LC = min(Ng, A.table_words / (2 * W));                 // levels of one pass
    const int *ang = A.angles + (size_t)R.ang * 3;
    const int alpha = A.alpha;
    for (int l0 = 0; l0 < Ng; l0 += LC) {
      const int lc = min(LC, Ng - l0);
      unsigned *Td = T, *Tn = T + lc * W;
      __syncthreads();
      for (int k = tid; k < 2 * lc * W; k += nthr) T[k] = 0;
      __syncthreads();
      for (int i = tid; i < nvox; i += nthr) {
        const int c = L[i];
        if (!c || (unsigned)(c - 1 - l0) >= (unsigned)lc) continue;
        const int z = i / plane, r = i - z * plane, y = r / nx, x = r - y * nx;
        int cnt = 0, sum = 0, dep = 0;
        for (int a = 0; a < na; a++) {
          const int dz = ang[3 * a], dy = ang[3 * a + 1], dx = ang[3 * a + 2];
          const int step = dz * plane + dy * nx + dx;
#pragma unroll
          for (int sgn = 0; sgn < 2; sgn++) {
            const int zz = sgn ? z - dz : z + dz, yy = sgn ? y - dy : y + dy, xx = sgn ? x - dx : x + dx;
            if ((unsigned)zz >= (unsigned)nz || (unsigned)yy >= (unsigned)ny || (unsigned)xx >= (unsigned)nx) continue;
            const int v = L[sgn ? i - step : i + step];
            if (!v) continue;
            cnt++;
            sum += v;
            dep += abs(c - v) <= alpha;
          }
        }
        const int row = (c - 1 - l0) * W;
        atomicAdd(&Td[row + dep], 1u);
        const int d = abs(cnt * c - sum);
        if (d) atomicAdd(&Tn[row + cnt], (unsigned)d);
      }
      __syncthreads();
      if (A.gldm) {   // [Ng][2 Nb + 1]: dependence counts reach Nb, the columns beyond stay zero (the reference's row stride)
        double *out = A.gldm + R.out[2] + (size_t)l0 * width;
        for (int k = tid; k < lc * width; k += nthr) {
          const int gl = k / width, col = k - gl * width;
          out[k] = col <= Nb ? (double)Td[gl * W + col] : 0.0;
        }
      }
      if (A.ngtdm) {  // [Ng][3]: voxels of the level, sum_c (sum over voxels with c neighbours) / c (ngtdm_finalize_kernel), level
        double *out = A.ngtdm + R.out[3] + (size_t)l0 * 3;
        for (int gl = tid; gl < lc; gl += nthr) {
          unsigned n = 0;
          double s = 0.0;
          for (int k = 0; k < W; k++) n += Td[gl * W + k];
          for (int k = 1; k < W; k++) s += (double)Tn[gl * W + k] / (double)k;
          out[gl * 3] = (double)n;
          out[gl * 3 + 1] = s;
          out[gl * 3 + 2] = (double)(l0 + gl + 1);
        }
      }
    }
  }
}

}  // namespace prad
