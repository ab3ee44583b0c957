// kernels_batch_firstorder.h -- the front end of the batched small-ROI route (gfx950): the first-order statistics and the
// discretisation of MANY small ROIs, one launch each, one workgroup of 256 threads per ROI.
//
// batch_firstorder_kernel<T>.  ROI b is a box of n = nz ny nx elements of T at element off[b] of the image buffer, its
// uint8 mask at the same element of the mask buffer.
//   compact   the box is streamed once, 256 elements per round; the values with mask != 0 go into LDS as order-preserving
//             unsigned keys (fo_key32 / fo_key: 4 bytes for float32, int32, int16, 8 bytes for float64).  A wave reserves
//             its slots with one LDS atomic on the cursor; where the waves' pieces land does not matter: they are sorted.
//             Slots beyond the capacity are counted, not stored (verdict 8); a non-finite value raises a flag (verdict 2).
//   sort      bitonic network over P = the next power of two >= min(n, capacity), padded with the largest key.  P follows
//             from the box size alone: every trip count of the kernel is fixed by the ROI record, none by image data.
//   order     Minimum / Maximum = keys[0] / keys[m - 1]; P10, P25, P75, P90 by fo_quantile_pos + fo_lerp_np, Median = the
//             middle element or the mean of the middle pair (fo_glue_quantiles_kernel's rule).
//   sums      over the SORTED keys, in float64: thread t adds elements t, t + 256, ... in index order, then fo_block_sum:
//             6 __shfl_xor steps and sh[0] + sh[1] + sh[2] + sh[3].  A term passes through at most ceil(m / 256) + 6 + 3
//             additions.  The sorted array is a function of the ROI's values alone, so a row depends neither on the order
//             the compaction's atomics landed in nor on the ROI's place in the batch.
//             pass 1: sum x, sum (x + shift)^2 -> Mean = sum x / m (one division)
//             pass 2: sum |d|, d^2, d^3, d^4 with d = x - Mean; count and sum of the band P10 <= x <= P90
//             pass 3: sum |x - band mean| over the band -> rMAD (NaN for an empty band)
//   row       16 doubles: the PRAD_FO_COUNT fields, then the verdict (0 fine, 1 empty ROI, 2 non-finite value, 8 more ROI
//             voxels than the capacity); the 15 fields are NaN unless the verdict is 0.
// LDS (dynamic, sized by the largest box of the launch; nothing static, so the key array stays 16-byte aligned):
//     PRAD_BFO_MISC_BYTES   64   cursor, non-finite flag, the four wave sums of fo_block_sum
//   + P * sizeof(key)            <= PRAD_BFO_KEY_BYTES = 128 KiB: 32768 four-byte keys or 16384 eight-byte keys
//   A batch of 16^3 boxes asks for 16 KiB + 64 and runs 8 workgroups per CU (the 32-wave limit); a 32^3 box takes a CU alone.
//
// batch_digitize_kernel<T>.  The ROI's edges (float64, built on the host by imageoperations.getBinEdges) are staged in LDS
// beside one counter per level; level = number of edges <= (double)x, found by a bisection of fixed length (the step count
// follows from the edge count in the ROI record) whose comparisons are those of digitize_kernel's level_of -- se[k] <= v on
// doubles; a NaN gives 0.  Every element of the int32 level box is written (0 outside the mask); the counts go to a flat int64
// buffer, nedges + 1 per ROI; top[b] = the largest level.
// LDS: 64 + 8 nedges + 4 (nedges + 1) rounded up to 16; PRAD_BATCH_DIGITIZE_MAX_EDGES = 8192 -> 96 KiB + 80.
#pragma once
#define PRAD_DEVICE_FUNCTIONS_ONLY      // fo_key / fo_unkey, fo_block_sum, fo_quantile_pos, fo_lerp_np: no second copy of the glue kernels
#include "kernels_firstorder.h"

namespace prad {

#define PRAD_BFO_THREADS 256
#define PRAD_BFO_MISC_BYTES 64
#define PRAD_BFO_KEY_BYTES (128 * 1024)
#define PRAD_BATCH_DIGITIZE_MAX_EDGES 8192
#define PRAD_BFO_VERDICT_EMPTY 1
#define PRAD_BFO_VERDICT_NONFINITE 2
#define PRAD_BFO_VERDICT_CAPACITY 8

static_assert(PRAD_BFO_MISC_BYTES + PRAD_BFO_KEY_BYTES <= 160 * 1024, "misc + keys fit the LDS of a CU");
static_assert(PRAD_BFO_MISC_BYTES % 16 == 0, "the key array is 16-byte aligned");
static_assert(PRAD_BFO_THREADS == 256, "four waves: fo_block_sum adds four wave sums");
static_assert(64 + 8 * PRAD_BATCH_DIGITIZE_MAX_EDGES + 4 * (PRAD_BATCH_DIGITIZE_MAX_EDGES + 1) + 12 <= 160 * 1024, "edges + counters fit the LDS of a CU");
static_assert(PRAD_BATCH_DIGITIZE_MAX_EDGES >= 4096 && (PRAD_BATCH_DIGITIZE_MAX_EDGES & (PRAD_BATCH_DIGITIZE_MAX_EDGES - 1)) == 0, "edge cap");

// the 32-bit analogue of fo_key / fo_unkey: unsigned keys in the order of the floats (-0.0 before +0.0)
__device__ __host__ __forceinline__ unsigned fo_key32(float x) {
  unsigned b;
  memcpy(&b, &x, sizeof(b));
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __host__ __forceinline__ float fo_unkey32(unsigned k) {
  const unsigned b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
  float x;
  memcpy(&x, &b, sizeof(x));
  return x;
}

// key type, key and value (widened to float64: exact) of every image dtype
template <typename T> struct BfoKey;
template <> struct BfoKey<float> {
  typedef unsigned key_t;
  static __device__ __forceinline__ key_t key(float x) { return fo_key32(x); }
  static __device__ __forceinline__ double value(key_t k) { return (double)fo_unkey32(k); }
  static __device__ __forceinline__ bool finite(float x) { return isfinite(x); }
};
template <> struct BfoKey<double> {
  typedef unsigned long long key_t;
  static __device__ __forceinline__ key_t key(double x) { return fo_key(x); }
  static __device__ __forceinline__ double value(key_t k) { return fo_unkey(k); }
  static __device__ __forceinline__ bool finite(double x) { return isfinite(x); }
};
template <> struct BfoKey<int> {
  typedef unsigned key_t;
  static __device__ __forceinline__ key_t key(int x) { return (unsigned)x ^ 0x80000000u; }
  static __device__ __forceinline__ double value(key_t k) { return (double)(int)(k ^ 0x80000000u); }
  static __device__ __forceinline__ bool finite(int) { return true; }
};
template <> struct BfoKey<short> {
  typedef unsigned key_t;
  static __device__ __forceinline__ key_t key(short x) { return (unsigned)(int)x ^ 0x80000000u; }
  static __device__ __forceinline__ double value(key_t k) { return (double)(int)(k ^ 0x80000000u); }
  static __device__ __forceinline__ bool finite(short) { return true; }
};

struct BatchFoRoi {
  long long off;       // first element of the box in the image / mask buffers
  long long n;         // elements of the box (< 2^31)
  int P;               // slots sorted: the next power of two >= min(n, capacity)
  int pad;
};

template <typename T>
__global__ void __launch_bounds__(PRAD_BFO_THREADS) batch_firstorder_kernel(const T *__restrict__ image,
                                                                            const uint8_t *__restrict__ mask,
                                                                            const BatchFoRoi *__restrict__ rois, int capacity,
                                                                            double shift, double *__restrict__ table) {
#pragma clang fp contract(off)
  typedef typename BfoKey<T>::key_t key_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char bfo_lds[];
  unsigned *misc = reinterpret_cast<unsigned *>(bfo_lds);                       // [0] cursor, [1] non-finite flag
  double *sh = reinterpret_cast<double *>(bfo_lds + 16);                        // [4]
  key_t *keys = reinterpret_cast<key_t *>(bfo_lds + PRAD_BFO_MISC_BYTES);       // [P]
  const BatchFoRoi r = rois[blockIdx.x];
  const T *x = image + r.off;
  const uint8_t *mk = mask + r.off;
  const int t = threadIdx.x, lane = t & 63;
  const int P = r.P;
  if (t < 2) misc[t] = 0u;
  __syncthreads();

  // ---- compact ------------------------------------------------------------------------------------------------------------
  const long long rounds = (r.n + PRAD_BFO_THREADS - 1) / PRAD_BFO_THREADS;
  bool bad = false;
  for (long long q = 0; q < rounds; q++) {
    const long long i = q * PRAD_BFO_THREADS + t;
    const bool in = i < r.n && mk[i] != 0;
    T v = T();
    if (in) v = x[i];
    const unsigned long long ball = __ballot(in);
    unsigned wbase = 0;
    if (lane == 0 && ball) wbase = atomicAdd(&misc[0], (unsigned)__popcll(ball));
    wbase = __shfl(wbase, 0);
    if (in) {
      const unsigned slot = wbase + (unsigned)__popcll(ball & ((1ull << lane) - 1ull));
      if (slot < (unsigned)capacity) keys[slot] = BfoKey<T>::key(v);      // (slot < capacity <= P: inside the array)
      bad = bad || !BfoKey<T>::finite(v);
    }
  }
  if (bad) misc[1] = 1u;
  __syncthreads();
  const unsigned total = misc[0];
  const bool nonfinite = misc[1] != 0u;
  double *row = table + (size_t)blockIdx.x * 16;
  int verdict = 0;
  if (total == 0u) verdict = PRAD_BFO_VERDICT_EMPTY;
  else if (total > (unsigned)capacity) verdict = PRAD_BFO_VERDICT_CAPACITY;
  else if (nonfinite) verdict = PRAD_BFO_VERDICT_NONFINITE;
  if (verdict) {                       // (the same for every thread of the workgroup)
    if (t < 15) row[t] = __builtin_nan("");
    if (t == 15) row[15] = (double)verdict;
    return;
  }
  const int m = (int)total;
  for (int i = m + t; i < P; i += PRAD_BFO_THREADS) keys[i] = ~(key_t)0;

  // ---- sort ---------------------------------------------------------------------------------------------------------------
  for (int size = 2; size <= P; size <<= 1) {
    for (int str = size >> 1; str > 0; str >>= 1) {
      __syncthreads();
      for (int k = t; k < (P >> 1); k += PRAD_BFO_THREADS) {
        const int i = ((k & ~(str - 1)) << 1) + (k & (str - 1)), j = i + str;      // (str is a power of two)
        const bool up = (i & size) == 0;
        const key_t a = keys[i], b = keys[j];
        if ((a > b) == up) {
          keys[i] = b;
          keys[j] = a;
        }
      }
    }
  }
  __syncthreads();

  // ---- order statistics (every thread: broadcast reads) ---------------------------------------------------------------------
  const double qs[5] = {0.1, 0.25, 0.5, 0.75, 0.9};
  double pq[5], mid[2] = {0.0, 0.0};
  for (int k = 0; k < 5; k++) {
    long long p, nx;
    double g;
    fo_quantile_pos((long long)m, qs[k], &p, &nx, &g);
    const double a = BfoKey<T>::value(keys[p]), b = BfoKey<T>::value(keys[nx]);
    pq[k] = fo_lerp_np(a, b, g);
    if (k == 2) { mid[0] = a; mid[1] = b; }
  }
  const double median = (m % 2) ? mid[0] : (mid[0] + mid[1]) / 2.0;
  const double vmin = BfoKey<T>::value(keys[0]), vmax = BfoKey<T>::value(keys[m - 1]);
  const double dm = (double)m;

  // ---- sums over the sorted array -------------------------------------------------------------------------------------------
  double s1 = 0, s2 = 0;
  for (int i = t; i < P; i += PRAD_BFO_THREADS)
    if (i < m) {
      const double v = BfoKey<T>::value(keys[i]), y = v + shift;
      s1 += v;
      s2 += y * y;
    }
  s1 = fo_block_sum(s1, sh);
  s2 = fo_block_sum(s2, sh);
  const double mu = s1 / dm;
  double a1 = 0, a2 = 0, a3 = 0, a4 = 0, bc = 0, bs = 0;
  for (int i = t; i < P; i += PRAD_BFO_THREADS)
    if (i < m) {
      const double v = BfoKey<T>::value(keys[i]);
      const double d = v - mu, d2 = d * d;
      a1 += fabs(d);
      a2 += d2;
      a3 += d2 * d;
      a4 += d2 * d2;
      if (v >= pq[0] && v <= pq[4]) {
        bc += 1.0;
        bs += v;
      }
    }
  a1 = fo_block_sum(a1, sh);
  a2 = fo_block_sum(a2, sh);
  a3 = fo_block_sum(a3, sh);
  a4 = fo_block_sum(a4, sh);
  bc = fo_block_sum(bc, sh);
  bs = fo_block_sum(bs, sh);
  const double mub = bc > 0 ? bs / bc : 0.0;
  double ba = 0;
  for (int i = t; i < P; i += PRAD_BFO_THREADS)
    if (i < m) {
      const double v = BfoKey<T>::value(keys[i]);
      if (v >= pq[0] && v <= pq[4]) ba += fabs(v - mub);
    }
  ba = fo_block_sum(ba, sh);
  if (t == 0) {
    row[PRAD_FO_NP] = dm;
    row[PRAD_FO_ENERGY] = s2;
    row[PRAD_FO_MINIMUM] = vmin;
    row[PRAD_FO_P10] = pq[0];
    row[PRAD_FO_P25] = pq[1];
    row[PRAD_FO_MEDIAN] = median;
    row[PRAD_FO_P75] = pq[3];
    row[PRAD_FO_P90] = pq[4];
    row[PRAD_FO_MAXIMUM] = vmax;
    row[PRAD_FO_MEAN] = mu;
    row[PRAD_FO_MAD] = a1 / dm;
    row[PRAD_FO_RMAD] = bc > 0 ? ba / bc : __builtin_nan("");
    row[PRAD_FO_M2] = a2 / dm;
    row[PRAD_FO_M3] = a3 / dm;
    row[PRAD_FO_M4] = a4 / dm;
    row[15] = 0.0;
  }
}

struct BatchDigRoi {
  long long off;       // first element of the box in the image / mask / level buffers
  long long n;         // elements of the box
  long long edges;     // first edge of the ROI in the flat edge buffer
  long long counts;    // first of its nedges + 1 counts; < 0: the ROI is not served by this launch (nothing is written)
  int nedges;          // 0: a ROI without edges (empty mask): every level is 0
  int step;            // the largest power of two <= max(nedges, 1): first step of the bisection
};

template <typename T>
__global__ void __launch_bounds__(PRAD_BFO_THREADS) batch_digitize_kernel(const T *__restrict__ image,
                                                                          const uint8_t *__restrict__ mask,
                                                                          const BatchDigRoi *__restrict__ rois,
                                                                          const double *__restrict__ edges,
                                                                          int *__restrict__ levels,
                                                                          long long *__restrict__ counts,
                                                                          int *__restrict__ top) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bdg_lds[];
  const BatchDigRoi r = rois[blockIdx.x];
  if (r.counts < 0) return;            // (the same for every thread of the workgroup)
  int *stop = reinterpret_cast<int *>(bdg_lds);                                // [4] wave maxima
  double *se = reinterpret_cast<double *>(bdg_lds + 64);                        // [nedges]
  unsigned *cnt = reinterpret_cast<unsigned *>(bdg_lds + 64 + 8 * (size_t)r.nedges);   // [nedges + 1]
  const int t = threadIdx.x;
  const int ne = r.nedges;
  for (int i = t; i < ne; i += PRAD_BFO_THREADS) se[i] = edges[r.edges + i];
  for (int i = t; i <= ne; i += PRAD_BFO_THREADS) cnt[i] = 0u;
  __syncthreads();
  const T *x = image + r.off;
  const uint8_t *mk = mask + r.off;
  int *lv = levels + r.off;
  int best = 0;
  for (long long i = t; i < r.n; i += PRAD_BFO_THREADS) {
    int k = 0;
    if (mk[i]) {
      const double v = (double)x[i];
      for (int s = r.step; s > 0; s >>= 1) {         // number of edges <= v (np.digitize); a NaN compares false: 0
        const int j = k + s;
        if (j <= ne && se[j - 1] <= v) k = j;
      }
      atomicAdd(&cnt[k], 1u);
      best = max(best, k);
    }
    lv[i] = k;
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  if ((t & 63) == 0) stop[t >> 6] = best;
  __syncthreads();
  for (int i = t; i <= ne; i += PRAD_BFO_THREADS) counts[r.counts + i] = (long long)cnt[i];
  if (t == 0) top[blockIdx.x] = max(max(stop[0], stop[1]), max(stop[2], stop[3]));
}

}  // namespace prad
